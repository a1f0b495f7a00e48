"""`smalt index` on a reference file with FASTQ records: smaltgpu_index_build_text_ex / smaltgpu_fasta_parse_ex with
SMALTGPU_TEXT_FASTQ, Index.from_fasta(..., fastq=True), parse_fasta(..., fastq=True) and `smaltgpu-map index`
(smalt_amd/csrc/smg_fastq_ref.hip).  Against the reference's own `smalt index` on the committed texts
(tests/golden/make_golden_fastq_ref.py and the FASTQ text of make_golden_fasta.py: md5 of its files), with the bytes of text per
workgroup forced down (SMALTGPU_FASTA_BLOCK) so that texts of 1 to 3 kB span many blocks; against Index.build on the sequences of
the Python model for texts whose block borders are placed by construction and for a random reference dressed as wrapped FASTQ; and
the program end to end."""
import gzip
import os
import subprocess

import pytest

import fasta_data as fd
import fastq_ref_data as fq
import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
REF_SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")
BLOCKS = ["64", "256", None]


def _set_block(monkeypatch, block):
    if block is None:
        monkeypatch.delenv("SMALTGPU_FASTA_BLOCK", raising=False)
    else:
        monkeypatch.setenv("SMALTGPU_FASTA_BLOCK", block)


def _files(ix, prefix):
    try:
        ix.save(prefix)
    finally:
        ix.close()
    return open(prefix + ".sma", "rb").read(), open(prefix + ".smi", "rb").read()


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b256", "default"])
def test_the_fastq_text_of_the_fasta_fixtures_gives_the_reference_files(block, monkeypatch, tmp_path):
    """the text the FASTA reader refuses (and keeps refusing without the flag)"""
    from smalt_amd import api
    _set_block(monkeypatch, block)
    entry = [e for e in fd.MANIFEST if e["tag"] == "fastq"][0]
    assert entry["ref_status"] == 0 and entry["names"] == ["r1", "r2 x"] and entry["lengths"] == [80, 64]
    text = fd.text_of(entry)
    ix = api.Index.from_fasta(text, 11, 2, 0, fastq=True)
    assert ix.parse_ms > 0 and ix.build_ms > 0
    pre = str(tmp_path / "ix")
    _files(ix, pre)
    assert gu.md5(pre + ".sma") == entry["sma_md5"]
    assert gu.md5(pre + ".smi") == entry["smi_md5"]
    with pytest.raises(api.SmaltGpuError) as ei:
        api.Index.from_fasta(text, 11, 2, 0).close()
    assert fd.CAUSE["fastq"] in str(ei.value)


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b256", "default"])
@pytest.mark.parametrize("entry", fq.ACCEPTED, ids=[e["tag"] for e in fq.ACCEPTED])
def test_committed_texts_give_the_reference_files(entry, block, monkeypatch, tmp_path):
    from smalt_amd import api
    _set_block(monkeypatch, block)
    text = fq.text_of(entry)
    pre = str(tmp_path / "ix")
    _files(api.Index.from_fasta(text, entry["k"], entry["s"], 0, fastq=True), pre)
    assert gu.md5(pre + ".sma") == entry["sma_md5"]
    assert gu.md5(pre + ".smi") == entry["smi_md5"]
    names, seqs, times = api.parse_fasta(text, 0, fastq=True)
    assert names == entry["names"]
    assert [len(q) for q in seqs] == entry["lengths"]
    assert (names, seqs) == fq.parse_model_fq(text)
    assert times["parse_ms"] > 0


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b256", "default"])
@pytest.mark.parametrize("entry", fq.REFUSED, ids=[e["tag"] for e in fq.REFUSED])
def test_refused_texts_are_refused_as_wrong_format(entry, block, monkeypatch):
    from smalt_amd import api
    _set_block(monkeypatch, block)
    text = fq.text_of(entry)
    with pytest.raises(api.SmaltGpuError) as ei:
        api.Index.from_fasta(text, entry["k"], entry["s"], 0, fastq=True).close()
    assert fq.WRONG in str(ei.value)
    with pytest.raises(api.SmaltGpuError) as ei:
        api.parse_fasta(text, 0, fastq=True)
    assert fq.WRONG in str(ei.value)


def test_a_refusal_names_the_record_its_prompt_and_its_offset(monkeypatch):
    from smalt_amd import api
    _set_block(monkeypatch, "64")
    text = fq.text_of([e for e in fq.MANIFEST if e["tag"] == "qual_short_at_end"][0])
    with pytest.raises(api.SmaltGpuError) as ei:
        api.parse_fasta(text, 0, fastq=True)
    msg = str(ei.value)
    assert "'s3'" in msg and "prompt 5 " in msg and "byte %d)" % text.index(b"@s3\n") in msg and "397 characters for 401 bases" in msg, msg


def test_a_text_handed_over_by_the_fasta_route_is_refused_and_the_next_one_read(monkeypatch):
    """the text begins with a '>' record, so the FASTA route runs first, finds the '@' and leaves the text in HBM for the walk over
    the records; the walk refuses the last record, whose quality line is one character short.  The next call in the same process,
    on the text with the quality repaired, goes the same way and is read."""
    import re
    import numpy as np
    from smalt_amd import api
    _set_block(monkeypatch, "64")
    rng = np.random.default_rng(99)
    head = b">fa one\n" + fq._rand(rng, 70) + b"\n" + fq._rand(rng, 45) + b"\n@s2 x\n" + fq._rand(rng, 90) + b"\n+\n" + fq._rand(rng, 90, fq.QUAL[1:30]) + b"\n"
    seq3, qual3 = fq._rand(rng, 130), fq._rand(rng, 130, fq.QUAL[1:30])
    bad, good = head + b"@s3\n" + seq3 + b"\n+\n" + qual3[:-1] + b"\n", head + b"@s3\n" + seq3 + b"\n+\n" + qual3 + b"\n"
    assert len(good) < 1000 and len(bad) > 5 * 64
    with pytest.raises(ValueError) as mi:
        fq.parse_model_fq(bad)
    name, m, n = re.fullmatch(re.escape(fq.WRONG) + r": record '(.*)' has (\d+) quality characters for (\d+) bases", str(mi.value)).groups()
    assert (name, m, n) == ("s3", "129", "130")
    with pytest.raises(api.SmaltGpuError) as ei:
        api.parse_fasta(bad, 0, fastq=True)
    msg = str(ei.value)
    assert fq.WRONG in msg and "record '%s'" % name in msg and "byte %d)" % bad.index(b"@s3\n") in msg and "%s characters for %s bases" % (m, n) in msg, msg
    names, seqs = fq.parse_model_fq(good)
    assert names == ["fa one", "s2 x", "s3"] and [len(s) for s in seqs] == [115, 90, 130]
    assert api.parse_fasta(good, 0, fastq=True)[:2] == (names, seqs)


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b256", "default"])
def test_plain_fasta_texts_give_the_same_files_with_the_flag(block, monkeypatch, tmp_path):
    from smalt_amd import api
    _set_block(monkeypatch, block)
    for entry in fd.ACCEPTED:
        text = fd.text_of(entry)
        want = _files(api.Index.from_fasta(text, entry["k"], entry["s"], 0), str(tmp_path / "want"))
        got = _files(api.Index.from_fasta(text, entry["k"], entry["s"], 0, fastq=True), str(tmp_path / "got"))
        assert got == want, entry["tag"]
        assert gu.md5(str(tmp_path / "got.sma")) == entry["sma_md5"] and gu.md5(str(tmp_path / "got.smi")) == entry["smi_md5"], entry["tag"]
        assert api.parse_fasta(text, 0, fastq=True)[:2] == api.parse_fasta(text, 0)[:2], entry["tag"]
    for entry in fd.REFUSED:
        if entry["expect"] != "fastq":                # the other refusals stay what they are
            with pytest.raises(api.SmaltGpuError) as ei:
                api.Index.from_fasta(fd.text_of(entry), entry["k"], entry["s"], 0, fastq=True).close()
            assert fd.CAUSE[entry["expect"]] in str(ei.value)


def test_empty_blank_and_dropped_texts_are_refused():
    from smalt_amd import api
    for text, cause in ((b"", "empty"), (b" \n\t\n\n", "no sequence"), (b"+only\nIIII\n+dropped\nJJJJ\n", "no sequence")):
        with pytest.raises(api.SmaltGpuError) as ei:
            api.Index.from_fasta(text, 11, 2, 0, fastq=True).close()
        assert cause in str(ei.value)


PLACED = fq.placed_texts(64)


@pytest.mark.parametrize("tag", sorted(PLACED), ids=sorted(PLACED))
def test_block_borders_placed_by_construction(tag, monkeypatch, tmp_path):
    """the byte with which a quality section reaches n, the '\\n' in front of a '+' prompt, the '+' itself, the '\\n' of the quality
    header line and a quality line's leading '@', each as the LAST and as the FIRST byte of a 64-byte block; a one-line quality
    longer than five blocks; the byte that reaches n as the last byte of the text"""
    from smalt_amd import api
    text = PLACED[tag]
    names, seqs = fq.parse_model_fq(text)
    assert len(seqs) == 4
    want = _files(api.Index.build(seqs, names, 11, 2, 0), str(tmp_path / "want"))
    for block in ("64", "128", None):
        _set_block(monkeypatch, block)
        assert api.parse_fasta(text, 0, fastq=True)[:2] == (names, seqs), block
        got = _files(api.Index.from_fasta(text, 11, 2, 0, fastq=True), str(tmp_path / "got"))
        assert got == want, block


def test_random_reference_as_wrapped_fastq(monkeypatch, tmp_path):
    from smalt_amd import api
    text, names, seqs = fq.wrapped_fastq(1, 100_000)
    assert 150_000 < len(text) < 300_000
    fa = str(tmp_path / "ref.fq")
    with open(fa, "wb") as f:
        f.write(text)
    for n, (k, s) in enumerate([(13, 6), (20, 13)]):
        _set_block(monkeypatch, ["4096", None][n])       # 4096: one tile per block; default: one block of many tiles
        want = _files(api.Index.build(seqs, names, k, s, 0), str(tmp_path / "want"))
        assert api.parse_fasta(fa, 0, fastq=True)[:2] == (names, seqs), (k, s)
        got = _files(api.Index.from_fasta(fa, k, s, 0, fastq=True), str(tmp_path / "got"))
        assert got == want, (k, s)
        if os.path.exists(REF_SMALT):
            pre = str(tmp_path / "ref")
            subprocess.run([REF_SMALT, "index", "-k", str(k), "-s", str(s), pre, fa], check=True, capture_output=True)
            assert got == (open(pre + ".sma", "rb").read(), open(pre + ".smi", "rb").read()), (k, s)


def test_program_indexes_fastq_files(tmp_path):
    """`smaltgpu-map index` on a FASTQ fixture and on its gzipped copy writes the reference's files; a text with a short quality
    exits with 1, names the cause and leaves no index files"""
    entry = [e for e in fq.MANIFEST if e["tag"] == "wrapped"][0]
    plain, gz = str(tmp_path / "ref.fq"), str(tmp_path / "copy.fq.gz")
    with open(plain, "wb") as f:
        f.write(fq.text_of(entry))
    with open(gz, "wb") as f:
        f.write(gzip.compress(fq.text_of(entry)))
    for n, fa in enumerate((plain, gz)):
        pre = str(tmp_path / ("built%d" % n))
        r = subprocess.run([PROG, "index", "-k", "11", "-s", "2", pre, fa], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert gu.md5(pre + ".sma") == entry["sma_md5"]
        assert gu.md5(pre + ".smi") == entry["smi_md5"]
    bad = str(tmp_path / "short.fq")
    with open(bad, "wb") as f:
        f.write(fq.text_of([e for e in fq.MANIFEST if e["tag"] == "qual_short_first"][0]))
    pre = str(tmp_path / "bad")
    r = subprocess.run([PROG, "index", "-k", "11", "-s", "2", pre, bad], capture_output=True)
    assert r.returncode == 1
    assert fq.WRONG in r.stderr.decode() and "'s1'" in r.stderr.decode() and "840 characters for 500 bases" in r.stderr.decode()
    assert not os.path.exists(pre + ".smi") and not os.path.exists(pre + ".sma")
