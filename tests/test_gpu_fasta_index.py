"""`smalt index` on the library: the text of a FASTA file parsed on the GPU (smalt_amd/csrc/smg_fasta.hip) in front of the index
construction -- smaltgpu_index_build_text, smaltgpu_fasta_parse, Index.from_fasta, `smaltgpu-map index`.  Against the reference's
own `smalt index` on the committed texts (tests/golden/make_golden_fasta.py: md5 of its files, names and lengths from its `.sma`),
with the bytes of text per workgroup forced down (SMALTGPU_FASTA_BLOCK) so that texts of 1 kB span many blocks; against
Index.build (pinned to the reference by tests/test_gpu_indexbuild.py) on texts whose block boundaries are placed by construction
and on random references in random dresses; and the program end to end.  Every text is a few kB to 200 kB."""
import gzip
import os
import subprocess

import pytest

import fasta_data as fd
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
@pytest.mark.parametrize("entry", fd.ACCEPTED, ids=[e["tag"] for e in fd.ACCEPTED])
def test_committed_texts_give_the_reference_files(entry, block, monkeypatch, tmp_path):
    from smalt_amd import api
    _set_block(monkeypatch, block)
    text = fd.text_of(entry)
    if entry["gz"]:                                  # as a gzipped file, through the path branch of from_fasta
        src = str(tmp_path / "in.fa.gz")
        with open(src, "wb") as f:
            f.write(gzip.compress(text))
    else:
        src = text
    ix = api.Index.from_fasta(src, entry["k"], entry["s"], 0)
    assert ix.parse_ms > 0 and ix.build_ms > 0
    pre = str(tmp_path / "ix")
    _files(ix, pre)
    assert gu.md5(pre + ".sma") == entry["sma_md5"]
    assert gu.md5(pre + ".smi") == entry["smi_md5"]
    names, seqs, times = api.parse_fasta(src, 0)
    assert names == entry["names"]
    assert [len(q) for q in seqs] == entry["lengths"]
    assert (names, seqs) == fd.parse_model(text)
    assert times["parse_ms"] > 0


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b256", "default"])
@pytest.mark.parametrize("entry", fd.REFUSED, ids=[e["tag"] for e in fd.REFUSED])
def test_refused_texts_name_their_cause(entry, block, monkeypatch):
    from smalt_amd import api
    _set_block(monkeypatch, block)
    with pytest.raises(api.SmaltGpuError) as ei:
        api.Index.from_fasta(fd.text_of(entry), entry["k"], entry["s"], 0).close()
    assert fd.CAUSE[entry["expect"]] in str(ei.value)


def test_empty_and_blank_texts_are_refused():
    from smalt_amd import api
    for text, cause in ((b"", "empty"), (b" \n\t\n\n", "no sequence")):
        with pytest.raises(api.SmaltGpuError) as ei:
            api.Index.from_fasta(text, 11, 2, 0).close()
        assert cause in str(ei.value)


BOUNDARY = fd.boundary_texts(64)


@pytest.mark.parametrize("tag", sorted(BOUNDARY), ids=sorted(BOUNDARY))
def test_block_boundaries_placed_by_construction(tag, monkeypatch, tmp_path):
    """a '\\n' with the prompt first in the next block, the '\\r' of a CRLF, the '>' itself, the last byte of a header line (and its
    newline) as the LAST byte of a 64-byte block; a header line longer than three blocks, a one-line sequence longer than five"""
    from smalt_amd import api
    text = BOUNDARY[tag]
    names, seqs = fd.parse_model(text)
    assert len(seqs) >= 2
    want = _files(api.Index.build(seqs, names, 11, 2, 0), str(tmp_path / "want"))
    for block in ("64", "128", None):
        _set_block(monkeypatch, block)
        assert api.parse_fasta(text, 0)[:2] == (names, seqs), block
        got = _files(api.Index.from_fasta(text, 11, 2, 0), str(tmp_path / "got"))
        assert got == want, block


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_references_in_random_dresses(seed, monkeypatch, tmp_path):
    from smalt_amd import api
    text, names, seqs = fd.dressed_reference(seed)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "wb") as f:
        f.write(text)
    for n, (k, s) in enumerate([(13, 6), (20, 13)]):
        _set_block(monkeypatch, ["4096", None][n])       # 4096: one tile per block, some 60 blocks; default: one block, 64 tiles
        want = _files(api.Index.build(seqs, names, k, s, 0), str(tmp_path / "want"))
        got = _files(api.Index.from_fasta(fa, k, s, 0), str(tmp_path / "got"))
        assert got == want, (k, s)
        if os.path.exists(REF_SMALT):
            pre = str(tmp_path / "ref")
            subprocess.run([REF_SMALT, "index", "-k", str(k), "-s", str(s), pre, fa], check=True, capture_output=True)
            assert got == (open(pre + ".sma", "rb").read(), open(pre + ".smi", "rb").read()), (k, s)


def test_program_index_then_map(oracle_built, tmp_path):
    """`smaltgpu-map index` on the .fa of a fixture and on its gzipped copy writes the reference's files; mapping through them prints
    what mapping through the fixture's own index files prints; a refused text exits with 1 and leaves no .smi"""
    entry = [e for e in gu.MANIFEST if e["tag"] == "g_k13s6_hash"][0]
    fx = gu.unpack(entry, tmp_path)
    gz = str(tmp_path / "copy.fa.gz")
    with open(gz, "wb") as f:
        f.write(gzip.compress(open(fx["fa"], "rb").read()))
    outs = []
    for n, fa in enumerate((fx["fa"], gz)):
        pre = str(tmp_path / ("built%d" % n))
        r = subprocess.run([PROG, "index", "-k", "13", "-s", "6", pre, fa], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert gu.md5(pre + ".sma") == entry["sma_md5"]
        assert gu.md5(pre + ".smi") == entry["smi_md5"]
    for prefix in (fx["prefix"], pre):
        out = str(tmp_path / "map.txt")
        r = subprocess.run([PROG, "-r", "7", "-o", out, prefix, fx["fq"]], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[0].count(b"\n") >= 250
    bad = str(tmp_path / "nohead.fa")
    with open(bad, "wb") as f:
        f.write(fd.text_of([e for e in fd.MANIFEST if e["tag"] == "nohead"][0]))
    pre = str(tmp_path / "bad")
    r = subprocess.run([PROG, "index", "-k", "11", "-s", "2", pre, bad], capture_output=True)
    assert r.returncode == 1
    assert fd.CAUSE["nohead"] in r.stderr.decode() and len(r.stderr.decode().strip().split("\n")) <= 2
    assert not os.path.exists(pre + ".smi") and not os.path.exists(pre + ".sma")
