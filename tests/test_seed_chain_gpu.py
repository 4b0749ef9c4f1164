"""The polishing chain with no outside tool: `hinge seed` -> `hinge paf2las --ends local` -> `hinge consensus` on cns_tiny, through the
executables.  Every read with a generator record of >= 400 contig bases must get a .las record on that record's contig and strand;
the consensus FASTA must be the reference program's on the same .las where it was built, else the CPU oracle's."""
import os
import subprocess

import pytest

import consensus_common as cc
from hinge_amd import formats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINGE = os.path.join(ROOT, "hinge_amd", "bin", "hinge")


def _run(cmd, wd):
    r = subprocess.run(cmd, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (cmd, r.stderr.decode()[-2000:])
    return r.stdout.decode(), r.stderr.decode()


def test_chain_seed_paf2las_consensus_cns_tiny(oracle_lib, tmp_path):
    wd = str(tmp_path)
    d = cc.make("cns_tiny", wd)
    os.remove(os.path.join(wd, "draft.reads.las"))                                 # the generator's own: the chain writes its own
    out, err = _run([HINGE, "seed", "draft", "reads", "x.paf"], wd)
    assert "%d reads," % len(d.reads) in out and "without a placement" in err and "OVERFLOW" in err
    lines = open(os.path.join(wd, "x.paf")).read().splitlines()
    assert "%d placements written" % len(lines) in out and len(lines) >= len(d.reads) - 4
    for ln in lines:
        f = ln.split("\t")
        assert len(f) == 14 and f[4] in "+-" and f[11] == "255" and f[12].startswith("sd:i:") and f[13] == "sc:i:" + f[9] and int(f[10]) == int(f[8]) - int(f[7])
    summary, _ = _run([HINGE, "paf2las", "draft", "reads", "x.paf", "draft.reads.las", "--ends", "local"], wd)
    assert "%d placements read" % len(lines) in summary
    las = formats.read_las(os.path.join(wd, "draft.reads.las"))
    have = {(int(r["bread"]), int(r["aread"]), int(r["flags"]) & 1) for r in las.rec}
    longest = {}
    for q in d.rec:
        b, ln = int(q["bread"]), int(q["aepos"]) - int(q["abpos"])
        if b not in longest or ln > longest[b][0]:
            longest[b] = (ln, int(q["aread"]), int(q["flags"]) & 1)
    need = [(b, a, c) for b, (ln, a, c) in sorted(longest.items()) if ln >= 400]
    assert len(need) >= 40 and [n for n in need if n not in have] == []
    hip, _ = _run([HINGE, "consensus", "draft", "reads", "draft.reads.las", "hip.fasta", "nominal.ini"], wd)
    fasta = open(os.path.join(wd, "hip.fasta"), "rb").read()
    assert fasta.count(b">Consensus") == len(d.contigs)
    ref = cc.run_reference(wd) or cc.run_oracle(oracle_lib, wd)                    # the reference's own program where it was built, else the restatement pinned to it
    assert fasta == ref[0] and hip.encode() == ref[1]                              # byte-identical FASTA and stdout
