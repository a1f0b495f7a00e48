"""The device stage of the index construction (build_index_device, smalt_amd/csrc/smg_indexbuild.hip) alone, at the shapes where its
kernels take another path: a sampling step above the word length (refusal and `maxpos` of the reference, tests/index_ref.py), the
grid-stride loops (SMALTGPU_INDEX_GRID caps the workgroups of every launch -- a knob for these tests only), the 32-bit-key path and its
switch to the hashed one, hundreds of sequence boundaries inside one workgroup, the packed words around the terminator, references
without any indexed word, the smallest hashed geometries, and a device pointer that is not word-aligned.

The reference data is the oracle's builder written with its writer (or_index_build / or_index_write, held to the reference program by
tests/test_index_ref.py and the golden fixtures); whole `.sma` and `.smi` files are compared byte for byte.  The first case of each
family also goes through the reference program where oracle/_ref/smalt was built.  Every case states the path it means to take
(index_ref.path) and is checked against the built index's own typ / nbits_key / nbits_lo.  Every reference is generated here."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import index_ref as ir
import oracle_lib as ol
from test_gpu_indexbuild import _messy_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
REF_SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")
KNOB = "SMALTGPU_INDEX_GRID"


def _names(seqs):
    return ["s%d" % i for i in range(len(seqs))]


def _read(prefix):
    return open(prefix + ".sma", "rb").read(), open(prefix + ".smi", "rb").read()


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _oracle_files(seqs, k, s, prefix):
    """the oracle's files, or None where its builder refuses"""
    n = len(seqs)
    names = [x.encode() for x in _names(seqs)]
    oix = ol.lib().or_index_build(n, (C.c_char_p * n)(*seqs), (C.c_uint32 * n)(*[len(q) for q in seqs]), (C.c_char_p * n)(*names), k, s)
    if not oix:
        return None
    try:
        assert ol.lib().or_index_write(oix, prefix.encode()) == 0
    finally:
        ol.lib().or_index_free(oix)
    return _read(prefix)


def _write_fasta(seqs, fn):
    with open(fn, "wb") as f:
        for name, q in zip(_names(seqs), seqs):
            f.write(b">" + name.encode() + b"\n" + q + b"\n")


def _reference_files(seqs, k, s, tmp_path):
    """the files of the reference's `smalt index`; None where the program is not built"""
    if not os.path.exists(REF_SMALT):
        return None
    fa, pre = str(tmp_path / "refprog.fa"), str(tmp_path / "refprog")
    _write_fasta(seqs, fa)
    subprocess.run([REF_SMALT, "index", "-k", str(k), "-s", str(s), pre, fa], check=True, capture_output=True)
    return _read(pre)


def _gpu_files(seqs, k, s, prefix, build=None):
    """files and description of the index the device builds"""
    from smalt_amd import api
    ix = build() if build else api.Index.build(seqs, _names(seqs), k, s, 0)
    try:
        d = ix.info()
        geo = (d.typ, d.nbits_key, d.nbits_lo)
        ix.save(prefix)
    finally:
        ix.close()
    return _read(prefix), geo


def _check(seqs, k, s, path, tmp_path, with_reference=False, build=None):
    """one reference through the oracle and the device: the path the case means to take, the geometry, both files -> the .smi header"""
    tot = sum(len(q) for q in seqs)
    assert ir.path(k, s, tot) == path, (k, s, tot)
    want = _oracle_files(seqs, k, s, str(tmp_path / "oracle"))
    assert want is not None
    got, geo = _gpu_files(seqs, k, s, str(tmp_path / "gpu"), build)
    assert geo == ir.geometry(k, s, tot), (k, s, tot)
    assert (geo[0] == ir.IDX_PERFECT) == (path == "k32")
    assert got[0] == want[0], ("sma", k, s, tot)
    assert got[1] == want[1], ("smi", k, s, tot)
    if with_reference:
        ref = _reference_files(seqs, k, s, tmp_path)
        if ref is not None:
            assert got == ref, ("reference program", k, s, tot)
    return ir.read_smi(str(tmp_path / "gpu.smi"))


# ---- 1. sampling step above the word length -------------------------------------------------------------------------------------------
TINY = ir.tiny_cases()


def _tiny_of(cls, n=10):
    out = [(k, s, seqs) for k, s, seqs in TINY if ir.classify([len(q) for q in seqs], k, s) == cls][:n]
    assert len(out) == n
    return out


def test_step_over_word_refused_references_name_the_sequence():
    from smalt_amd import api
    for k, s, seqs in _tiny_of("refused"):
        bad, _ = ir.carry([len(q) for q in seqs], k, s)
        with pytest.raises(api.SmaltGpuError) as ei:
            api.Index.build(seqs, _names(seqs), k, s, 0).close()
        assert ei.value.code == -3                                 # SMALTGPU_EARG
        assert "the reference refuses" in str(ei.value) and "sequence %d:" % bad in str(ei.value), (k, s, str(ei.value))


@pytest.mark.parametrize("cls", ["over", "grid"])
def test_step_over_word_built_references_give_the_reference_files(cls, oracle_built, tmp_path):
    """ten references the reference builds with `maxpos` one above the grid's, ten with the grid's: maxpos is word 3 of the .smi header"""
    for n, (k, s, seqs) in enumerate(_tiny_of(cls)):
        lens = [len(q) for q in seqs]
        smi = _check(seqs, k, s, ir.path(k, s, sum(lens)), tmp_path, with_reference=(n == 0))
        assert smi["maxpos"] == ir.carry(lens, k, s)[1] == ir.grid_maxpos(lens, s) + (1 if cls == "over" else 0)
        assert sorted(smi["pos"]) == ir.grid_positions(seqs, k, s)


def test_step_over_word_through_the_program(oracle_built, tmp_path):
    """`smaltgpu-map index`: a refused reference exits with 1 and leaves neither file; one with maxpos over the grid gives the files
    of the reference program (of the oracle where that program is not built)"""
    k, s, seqs = _tiny_of("refused", 1)[0]
    fa, pre = str(tmp_path / "bad.fa"), str(tmp_path / "bad")
    _write_fasta(seqs, fa)
    r = subprocess.run([PROG, "index", "-k", str(k), "-s", str(s), pre, fa], capture_output=True)
    assert r.returncode == 1 and "the reference refuses" in r.stderr.decode(), r.stderr.decode()[-2000:]
    assert not os.path.exists(pre + ".smi") and not os.path.exists(pre + ".sma")
    k, s, seqs = _tiny_of("over", 1)[0]
    fa, pre = str(tmp_path / "over.fa"), str(tmp_path / "over")
    _write_fasta(seqs, fa)
    r = subprocess.run([PROG, "index", "-k", str(k), "-s", str(s), pre, fa], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    want = _reference_files(seqs, k, s, tmp_path) or _oracle_files(seqs, k, s, str(tmp_path / "oracle"))
    assert (gu.md5(pre + ".sma"), gu.md5(pre + ".smi")) == (hashlib.md5(want[0]).hexdigest(), hashlib.md5(want[1]).hexdigest())
    assert ir.read_smi(pre + ".smi")["maxpos"] == ir.grid_maxpos([len(q) for q in seqs], s) + 1


# ---- 2. the grid-stride loops ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,path", [(8, 1, "k32"), (13, 6, "hash"), (20, 13, "hash")], ids=lambda v: str(v))
def test_strided_loops_on_a_messy_reference(k, s, path, oracle_built, monkeypatch, tmp_path):
    """one and three workgroups per launch against the default on 40 kb: every kernel's loop runs many times, k_ib_kmers with lanes that
    leave through its `continue` between the two barriers in the last round"""
    seqs = _messy_reference(40 + k, 3, 12_500, 14_001)
    for n, grid in enumerate((None, "1", "3")):
        if grid is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, grid)
        _check(seqs, k, s, path, tmp_path, with_reference=(n == 0 and k == 8))


@pytest.mark.parametrize("k,s,path", [(8, 1, "hash"), (13, 6, "hash"), (6, 1, "k32")], ids=lambda v: str(v))
def test_one_workgroup_at_the_ends_of_its_rounds(k, s, path, oracle_built, monkeypatch, tmp_path):
    """one workgroup: 255, 256 and 257 serials (the second round holds no serial, or one), and 2559, 2560, 2561 bases (the terminator is
    the last letter of the first round's words, or the first of the second round's)"""
    monkeypatch.setenv(KNOB, "1")
    rng = np.random.default_rng(5 + k)
    for tot in [255 * s, 256 * s, 257 * s, 256 * s - 1, 256 * s + 1, 2559, 2560, 2561]:
        _check([_acgt(rng, tot)], k, s, path if (k, s) != (6, 1) or tot >= 2048 else "hash", tmp_path)


def test_the_knob_ignores_what_is_no_number_in_range(oracle_built, monkeypatch, tmp_path):
    seqs = [_acgt(np.random.default_rng(3), 3000)]
    for v in ("0", "65537", "x", "3x", "", "-1"):
        monkeypatch.setenv(KNOB, v)
        _check(seqs, 11, 2, "hash", tmp_path)


# ---- 3. the 32-bit-key path and its switch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,tot", [(4, 1, 40_000), (4, 4, 40_000), (6, 3, 40_000), (8, 1, 40_000), (10, 1, 600_000), (11, 1, 2_200_000)],
                         ids=lambda v: str(v))
def test_perfect_indexes_on_the_32_bit_key_path(k, s, tot, oracle_built, tmp_path):
    """the sentinel 4^k behind every key, the sort over 2k + 1 bits, run ends and the count by atomics; (11, 1): 4^11 <= 2 * ntup only
    from 2.1 Mb on"""
    seqs = _messy_reference(300 + k + s, 4, tot // 4, tot // 4 + 1)
    smi = _check(seqs, k, s, "k32", tmp_path, with_reference=(k == 4 and s == 1))
    assert smi["npos"] > tot // s // 2


def test_the_switch_between_the_perfect_and_the_hashed_type(oracle_built, tmp_path):
    """(8, 3): 4^8 = 2 * 32768, so 98304 bases give a perfect index and 98303 a hashed one"""
    seq = _messy_reference(77, 1, 98_304, 98_305)[0]
    assert _check([seq], 8, 3, "k32", tmp_path, with_reference=True)["typ"] == ir.IDX_PERFECT
    assert _check([seq[:-1]], 8, 3, "hash", tmp_path, with_reference=True)["typ"] == ir.IDX_HASH32MIX


# ---- 4. many short sequences ----------------------------------------------------------------------------------------------------------
def _short_seqs(rng, n, k, s):
    return [_acgt(rng, int(rng.integers(k, k + 2 * s + 1))) for _ in range(n)]


SHORT = [(13, 6, "hash"), (11, 2, "hash"), (8, 8, "hash"), (20, 13, "hash"), (6, 3, "k32")]


@pytest.mark.parametrize("k,s,path", SHORT, ids=lambda v: str(v))
def test_three_thousand_short_sequences(k, s, path, oracle_built, tmp_path):
    """sequences of k .. k + 2s bases: the 256 serials of a workgroup span dozens of sequences, some without any grid point, so the
    workgroup's search is the answer for few lanes only; alone and between two sequences of 50 kb"""
    rng = np.random.default_rng(1000 + k)
    short = _short_seqs(rng, 3000, k, s)
    smi = _check(short, k, s, path, tmp_path, with_reference=(k == 13))
    assert sorted(smi["pos"]) == ir.grid_positions(short, k, s)
    _check([_acgt(rng, 50_000)] + short + [_acgt(rng, 50_001)], k, s, path, tmp_path)


@pytest.mark.parametrize("k,s,path", SHORT, ids=lambda v: str(v))
def test_sequences_that_end_at_or_just_before_a_word_end(k, s, path, oracle_built, tmp_path):
    """3000 sequences of exactly k bases; 1500 sequences whose last sampled word ends on their last base, alternating with ones that
    are one base short of that (g + k <= end of the sequence decides)"""
    rng = np.random.default_rng(2000 + k)
    exact = [_acgt(rng, k) for _ in range(3000)]
    smi = _check(exact, k, s, path, tmp_path)
    assert sorted(smi["pos"]) == ir.grid_positions(exact, k, s)
    seqs, base, fits = [], 0, 0
    for i in range(1500):
        g = (base + s - 1) // s * s + int(rng.integers(1, 4)) * s           # a grid point inside the sequence, not its first
        n = g + k - base - (i & 1)
        fits += 1 - (i & 1)
        seqs.append(_acgt(rng, n))
        base += n
    smi = _check(seqs, k, s, path, tmp_path)
    pos = ir.grid_positions(seqs, k, s)
    assert sorted(smi["pos"]) == pos
    ends = set(np.cumsum([len(q) for q in seqs]).tolist())
    assert sum(1 for t in pos if t * s + k in ends) == fits


# ---- 5. packing and the ends of the reference -----------------------------------------------------------------------------------------
def test_packed_words_around_the_terminator(oracle_built, tmp_path):
    """(3, 1): the terminator opens a word of its own (tot = 10, 20, 2560, 5120), is a word's last letter (9, 19, 2559) or its
    second (11, 21, 2561); at 2560 and 5120 it is the first letter of another workgroup's words"""
    rng = np.random.default_rng(11)
    for n, tot in enumerate([9, 10, 11, 19, 20, 21, 2559, 2560, 2561, 5120]):
        _check([_acgt(rng, tot)], 3, 1, "k32" if tot >= 32 else "hash", tmp_path, with_reference=(n == 0))


@pytest.mark.parametrize("two", [False, True], ids=["alone", "first_of_two"])
def test_reference_ends_around_a_workgroups_span(two, oracle_built, tmp_path):
    """(13, 6): tot = 256 * s * m + j: the last serials of the reference are the last of a workgroup or the first of the next, with a
    last word that fits by one base or misses by one; the same lengths with another sequence behind"""
    rng = np.random.default_rng(12)
    k, s = 13, 6
    for m in (1, 2):
        for j in (-1, 0, 1, k - 1, k):
            seqs = [_acgt(rng, 256 * s * m + j)] + ([_acgt(rng, 500)] if two else [])
            smi = _check(seqs, k, s, "hash", tmp_path)
            assert sorted(smi["pos"]) == ir.grid_positions(seqs, k, s)


def test_letters_on_the_first_and_the_last_base(oracle_built, tmp_path):
    """lower case, U, IUPAC letters and N as the first and as the last letter of the reference and of a sequence inside it"""
    rng = np.random.default_rng(13)
    for k, s, path in ((13, 6, "hash"), (6, 1, "k32")):
        for ch in b"aunNRYtg":
            seqs = []
            for n in (2560, 2559, 3001):
                q = bytearray(_acgt(rng, n))
                q[0] = q[-1] = ch
                seqs.append(bytes(q))
            smi = _check(seqs, k, s, path, tmp_path)
            assert sorted(smi["pos"]) == ir.grid_positions(seqs, k, s)


# ---- 6. nothing to index --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,k,s,path,npos", [(b"N" * 500, 11, 2, "hash", 0), (b"N" * 5000, 4, 1, "k32", 0),
                                               (b"ACGT" * 50 + b"N" * 300 + b"ACGGT" * 40, 11, 2, "hash", 190)],
                         ids=["hash_empty", "k32_empty", "hash_190"])
def test_references_with_no_or_few_indexed_words(seq, k, s, path, npos, oracle_built, tmp_path):
    """zero-length scans, sorts and allocations on both paths; the reference program builds these too"""
    smi = _check([seq], k, s, path, tmp_path, with_reference=True)
    assert smi["npos"] == npos and len(ir.grid_positions([seq], k, s)) == npos
    if npos == 0 and path == "hash":
        assert smi["nwords"] == 0


@pytest.mark.parametrize("seq,k,s", [(b"N" * 500, 11, 2), (b"N" * 5000, 4, 1)], ids=["hash", "k32"])
def test_mapping_through_an_empty_index_maps_nothing(seq, k, s):
    from smalt_amd import api
    rng = np.random.default_rng(14)
    reads = [_acgt(rng, 60) for _ in range(10)]
    ix = api.Index.build([seq], ["n"], k, s, 0)
    try:
        mp = api.Mapper(ix, 16, 64)
        try:
            res, _ = mp.map_batch(reads, [b"I" * len(r) for r in reads], ix.default_params())
        finally:
            mp.close()
    finally:
        ix.close()
    assert len(res) == 10 and all(len(r) == 0 for r in res)


# ---- 7. small hashed geometries -------------------------------------------------------------------------------------------------------
def test_small_hashed_geometries(oracle_built, tmp_path):
    """nbits_key down to 2 (three sequences of 13 bases at (13, 6)); nbits_lo 2 .. 8 with k = 17 .. 20 on 2 kb; (20, 127) on 15.6 kb,
    where nbits_key = nbits_lo + 1 = 9: one bit of the key comes from the hash"""
    rng = np.random.default_rng(15)
    seqs = [_acgt(rng, 13) for _ in range(3)]
    smi = _check(seqs, 13, 6, "hash", tmp_path, with_reference=True)
    assert (smi["nbits_key"], smi["nbits_lo"]) == (2, 0) and sorted(smi["pos"]) == ir.grid_positions(seqs, 13, 6)
    ref = _messy_reference(16, 1, 2000, 2001)
    for k in (17, 18, 19, 20):
        smi = _check(ref, k, 13, "hash", tmp_path)
        assert smi["nbits_lo"] == 2 * k - 32 and smi["nbits_key"] == max(6, smi["nbits_lo"] + 1)
    ref = [_acgt(rng, 15_600)]
    smi = _check(ref, 20, 127, "hash", tmp_path, with_reference=True)
    assert (smi["nbits_key"], smi["nbits_lo"]) == (9, 8)
    assert smi["maxpos"] == ir.carry([15_600], 20, 127)[1]


# ---- 8. a device pointer that is not word-aligned -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,path", [(8, 1, "k32"), (13, 6, "hash")], ids=lambda v: str(v))
def test_device_pointer_at_every_byte_offset(k, s, path, oracle_built, tmp_path):
    """the reference inside a device buffer at byte offsets 0 .. 3: the word-wise arm of the staging loop at 0, the byte-wise at 1 .. 3"""
    import torch
    from smalt_amd import api
    seqs = _messy_reference(80 + k, 3, 12_500, 14_001)
    cat = b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(q) for q in seqs])]).tolist()
    for o in range(4):
        host = torch.full((len(cat) + 8,), ord("A"), dtype=torch.uint8)
        host[o:o + len(cat)] = torch.frombuffer(bytearray(cat), dtype=torch.uint8)
        dev = host.to("cuda:0")
        torch.cuda.synchronize()
        assert dev.data_ptr() % 4 == 0
        _check(seqs, k, s, path, tmp_path, with_reference=(o == 1 and k == 13),
               build=lambda: api.Index.build_device(dev.data_ptr() + o, off, _names(seqs), k, s, 0))
        del dev
