"""`hinge fasta2db`: the FASTA -> DB writer through the dispatcher, read back by formats.read_db_index / read_bases and, where
oracle/_ref was built, by the reference's own Open_DB + Load_Read."""
import ctypes
import os
import subprocess

import numpy as np

HINGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hinge_amd", "bin", "hinge")

FASTA = """>ctg0 a comment
ACGTACGTAC
acgtacgtac
ACGTA
>ctg1
ttttggggccccaaaa

>ctg2
ACGNNNACGT
TTGCA
>ctg3
G
"""
WANT = ["ACGTACGTACACGTACGTACACGTA", "TTTTGGGGCCCCAAAA", "ACGAAAACGTTTGCA", "G"]       # (N is stored as A, as fasta2DB stores it)


def _fasta2db(tmp_path):
    wd = str(tmp_path)
    with open(os.path.join(wd, "in.fasta"), "w") as f:
        f.write(FASTA)
    r = subprocess.run([HINGE, "fasta2db", "in.fasta", "draft"], cwd=wd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    return os.path.join(wd, "draft")


def test_fasta2db_round_trip(tmp_path):
    from hinge_amd import formats
    db = _fasta2db(tmp_path)
    idx = formats.read_db_index(db)
    assert idx["rlen"].tolist() == [len(s) for s in WANT] and idx["treads"] == idx["ureads"] == len(WANT)
    got = ["".join("ACGT"[b] for b in r) for r in formats.read_bases(db, idx)]
    assert got == WANT
    # usage: two arguments, exit code 1 otherwise; a missing file is an error, not a traceback
    r = subprocess.run([HINGE, "fasta2db", "in.fasta"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"usage: hinge fasta2db" in r.stderr
    r = subprocess.run([HINGE, "fasta2db", "absent.fasta", "x"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"Traceback" not in r.stderr


def test_fasta2db_through_the_references_open_db(ref_lib, tmp_path):
    """The reference's own DB.c reads the written DB: Open_DB + Trim_DB give the lengths, Load_Read the bases."""
    db = _fasta2db(tmp_path)
    out = np.zeros(len(WANT), np.int32)
    assert ref_lib.ref_read_lengths(db.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(WANT)) == len(WANT)
    assert out.tolist() == [len(s) for s in WANT]
    hits_db = ctypes.create_string_buffer(512)          # HITS_DB is 112 bytes (formats.HITS_DB_SIZE)
    ref_lib.Open_DB.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    ref_lib.Trim_DB.argtypes = [ctypes.c_void_p]
    ref_lib.Load_Read.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    ref_lib.Close_DB.argtypes = [ctypes.c_void_p]
    assert ref_lib.Open_DB(db.encode(), hits_db) == 0
    ref_lib.Trim_DB(hits_db)
    buf = ctypes.create_string_buffer(64)
    for i, want in enumerate(WANT):
        assert ref_lib.Load_Read(hits_db, i, ctypes.addressof(buf) + 1, 2) == 0        # 2: upper-case letters; writes read[-1] and read[len] too
        assert buf.raw[1:1 + len(want)].decode() == want
    ref_lib.Close_DB(hits_db)
