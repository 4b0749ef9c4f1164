"""What tests/spec_model.py answers on the hand-made part of tests/wide_keys_common.py - the expected tables of
tests/test_wide_keys_gpu.py - and that the part is what it is for: one ungated annotation on read 0 whose decision sorts keys
spanning 2^20 or more (the supporters at S = 40, the pile-up too at S = 100)."""
import numpy as np
import pytest

import wide_keys_common as wk


@pytest.mark.parametrize("shape", wk.SHAPES)
@pytest.mark.parametrize("S", [40, 100])
def test_model_on_the_wide_key_part(oracle_lib, S, shape):
    from hinge_amd.config import default_filter_params
    part = wk.make_part(S, shape)
    m = wk.model(part, default_filter_params(), oracle_lib)
    assert m["min_cov"] == 9
    assert m["mask"].tolist() == [[320, wk.RLEN0 - 320]] + [[320, wk.RLEN - 320]] * S
    assert m["annos"][0] == [wk.ANNO] and not m["gated"][0]
    assert all(m["annos"][i] == [] and m["hinges"][i] == [] for i in range(1, S + 1))
    assert m["hinges"][0] == ([wk.ANNO] if shape == "hinge" else [])
    pile, sup = m["sorts"]                          # read 0: its pile-up by length sum, then the one annotation's supporters
    assert len(pile) == 45 + S and len(sup) == S
    assert wk.span(sup) == 1614400 >= 1 << 20       # the second hand-off: the supporter sort (always run by the LEAN instance)
    lens = pile[np.isin(part[2][:len(pile), 1], [wk.ANNO[0] + 20])]
    assert len(lens) == S and len(set(lens.tolist())) == S, "no length tie among the supporters"
    assert wk.span(pile) == 2340000 >= 1 << 20      # the first hand-off at S = 100: above 64 supporters the pile-up itself is sorted
