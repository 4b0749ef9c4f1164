"""`hinge overlap` in front of the chain: a noisy synth_draft set (size class draft_noisy, the genome shrunk to 30 kb) through
overlap -> filter -> maximal -> layout -> clip -> draft-path -> draft with the executables, and the same chain on the generator's own
.las beside it.  Every stage exits 0, both drafts have the same number of contigs, and the draft's identity with the planted genome
(chain_common.ContigOnGenome) on overlap's .las is no lower than on the generator's minus half the gap between that value and the
identity of a single raw read: a draft that overlap's records had spoilt half-way back to a raw read fails.
Measured on an MI355X: see DESIGN.md 3.11."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import chain_common as ch
import draft_common as dc
from hinge_amd import synth_draft as sd

pytestmark = pytest.mark.gpu

BIN = os.path.join(dc.ROOT, "hinge_amd", "bin")
SPEC = dataclasses.replace(sd.CONFIGS["draft_noisy"], genome_len=30_000)


def _chain(wd, d, overlap):
    """The executables on the data set in wd; overlap: G.las comes from `hinge overlap` instead of the generator.  Returns the draft FASTA."""
    from hinge_amd import clip, draft_path
    os.makedirs(wd, exist_ok=True)
    sd.write_dataset(d, wd, "G")
    with open(os.path.join(wd, "nominal.ini"), "w") as f:
        f.write(dc.DRAFT_INI)
    if overlap:
        os.remove(os.path.join(wd, "G.las"))
        r = subprocess.run([os.path.join(BIN, "hinge"), "overlap", "G", "G.las"], cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, ("overlap", r.stderr.decode()[-1500:])
        print(r.stdout.decode().strip())
    for prog, extra in (("Reads_filter", []), ("get_maximal_reads", []), ("hinging", ["-o", "G"])):
        r = subprocess.run([os.path.join(BIN, prog), "--db", "G", "--las", "G.las", "-x", "G", "--config", "nominal.ini"] + extra, cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (prog, r.stderr.decode()[-1500:])
    old = os.getcwd()
    os.chdir(wd)
    try:
        assert clip.main(["G.edges.hinges", "G.hinge.list", ".clip", "nominal.ini"]) == 0
        assert draft_path.main([".", "G", "G.clip.G2.graphml"]) == 0
    finally:
        os.chdir(old)
    return dc.run_product(wd)[0]


def _identity(d, fasta):
    """(contigs, equal columns / alignment columns over all contigs of 2 kb or more)."""
    ctgs = [s for _, s in dc.contigs_of(fasta)]
    placed = [ch.ContigOnGenome(ch.to_bases(s), d.genome) for s in ctgs if len(s) >= 2000]
    cols = sum(p.columns for p in placed)
    return len(ctgs), sum(p.identity * p.columns for p in placed) / max(cols, 1)


def test_chain_on_overlaps_las_beside_the_generators(tmp_path):
    d = sd.generate(SPEC)
    n_gen, id_gen = _identity(d, _chain(os.path.join(str(tmp_path), "gen"), d, False))
    n_ovl, id_ovl = _identity(d, _chain(os.path.join(str(tmp_path), "ovl"), d, True))
    raw = float(np.median([ch.ContigOnGenome(d.reads[r], d.genome).identity for r in range(0, len(d.reads), max(len(d.reads) // 8, 1))]))
    print("contigs: generator %d, overlap %d; identity: generator %.5f, overlap %.5f, a raw read %.5f" % (n_gen, n_ovl, id_gen, id_ovl, raw))
    assert n_gen >= 1 and n_ovl == n_gen
    assert id_gen > raw
    assert id_ovl >= id_gen - 0.5 * (id_gen - raw)
