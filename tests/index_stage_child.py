"""Child process of tests/test_index_stages_gpu.py: one stage (overlap | seed) in a fresh process, so that HINGE_INDEX_DEVICE is
read from this process's environment; every output array and the stats go to an .npz file.
    python index_stage_child.py overlap|seed WORKDIR OUT.npz"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main(stage, wd, out):
    from hinge_amd import capi, formats
    ctx = capi.Context(0)
    res, stats = {}, {}
    os.makedirs(wd, exist_ok=True)
    if stage == "overlap":
        import overlap_common as oc
        reads, _ = oc.edge_reads()
        formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in reads], np.int32), bases=reads)
        capi.Consensus(ctx, os.path.join(wd, "reads"), os.path.join(wd, "reads"))
        for label, kw in oc.edge_calls():
            if label not in ("defaults", "three_blocks", "max_occ2"):
                continue
            for x, a in enumerate(ctx.overlap_run(**kw)):
                res["%s_%d" % (label, x)] = a
            stats[label] = [ctx.overlap_stats(), ctx.index_last_stats()]
    else:
        from hinge_amd import synth_consensus as sc
        d = sc.generate(sc.CONFIGS["cns_tiny"])
        formats.write_db(os.path.join(wd, "draft"), np.asarray([len(c) for c in d.contigs], np.int32), bases=d.contigs)
        formats.write_db(os.path.join(wd, "reads"), np.asarray([len(r) for r in d.reads], np.int32), bases=d.reads)
        capi.Consensus(ctx, os.path.join(wd, "draft"), os.path.join(wd, "reads"))
        for label, kw in (("n1", dict()), ("n2_k10_occ1", dict(max_placements=2, k=10, max_occ=1))):
            for x, a in enumerate(ctx.seed_run(**kw)):
                res["%s_%d" % (label, x)] = a
            stats[label] = [ctx.seed_stats(), ctx.index_last_stats()]
    ctx.close()
    np.savez(out, stats=np.asarray(json.dumps(stats)), **res)


if __name__ == "__main__":
    main(*sys.argv[1:4])
