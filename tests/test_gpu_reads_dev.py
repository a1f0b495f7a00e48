"""FASTQ / FASTA read files parsed on the device (smaltgpu_reads_parse_device, smalt_amd/csrc/smg_reads_dev.hip) against the host
parser's general rules (smaltgpu_reads_parse through reads_dev_data.host_line): the corpus of tests/reads_dev_data.py whole and by
the chunk protocol, random texts, max_reads, the arrays as they lie in HBM with a guard behind each, a batch mapped straight from
the device view, two parses on one handle, and a text whose chain of records needs more than 16 jump tables."""
import ctypes as C
import gzip
import math
import os

import pytest

import golden_util as gu
import reads_dev_data as rd

pytestmark = pytest.mark.gpu
GUARD = 64
CHUNKS = [1, 63, 64, 65, 4097, rd.BLOCK - 1, rd.BLOCK, rd.BLOCK + 1]


@pytest.fixture(scope="module")
def dev():
    from smalt_amd import api
    d = api.ReadsDevice(0)
    d.configure(rd.BLOCK, 0, GUARD)          # the placed cases of the corpus are built around this block size
    yield d
    d.close()


def dev_line(d, text, is_last=True, max_reads=0, arrays=True):
    """the device parser's result in the form of host_line; arrays: what lies in HBM is the host view, the guards are whole"""
    from smalt_amd import api
    try:
        hv, dv = d.parse_raw(text, is_last, max_reads)
    except api.SmaltGpuError as e:
        assert e.code == rd.EFILE, e.args
        return "ERR " + api.lib().smaltgpu_last_error().decode("latin-1"), 0
    assert (dv.nreads, dv.has_qual, dv.consumed) == (hv.nreads, hv.has_qual, hv.consumed)
    assert dv.total_bases == hv.read_off[hv.nreads] and bool(dv.d_quals) == bool(hv.has_qual) and dv.d_bases and dv.d_read_off
    if arrays:
        n, tot = hv.nreads, int(dv.total_bases)
        bases, g0, _ = d.readback(0)
        quals, g1, _ = d.readback(1)
        offs, g2, _ = d.readback(2)
        assert g0 == g1 == g2 == b"\xa5" * GUARD
        assert bases == (C.string_at(hv.bases, tot) if tot else b"")
        assert quals == (C.string_at(hv.quals, tot) if (tot and hv.has_qual) else b"")
        assert offs == b"".join(int(hv.read_off[i]).to_bytes(8, "little") for i in range(n + 1)) and offs[:8] == bytes(8)
    return rd.view_line(hv), hv.consumed


@pytest.mark.parametrize("tag", sorted(rd.CORPUS), ids=sorted(rd.CORPUS))
def test_corpus_whole(tag, dev):
    text, is_last, _, rule = rd.CORPUS[tag]
    rd.check_case(tag)
    assert dev_line(dev, text, is_last) == rd.host_line(text, is_last), (tag, rule)


@pytest.mark.parametrize("chunk", CHUNKS, ids=["c%d" % c for c in CHUNKS])
def test_corpus_by_the_chunk_protocol(chunk, dev):
    """every call of the protocol sees the same buffer on both sides as long as `consumed` agrees, so the lines are compared call
    by call; texts of more than 150 chunks are left to the larger chunk sizes"""
    ran = 0
    for tag in sorted(rd.CORPUS):
        text = rd.CORPUS[tag][0]
        if len(text) > 150 * chunk:
            continue
        want = rd.chunk_calls(lambda b, last: rd.host_line(b, last), text, chunk)
        got = rd.chunk_calls(lambda b, last: dev_line(dev, b, last, arrays=False), text, chunk)
        assert got == want, (tag, chunk, len(got), len(want))
        ran += 1
    assert ran >= 20


def test_random_texts(dev):
    texts = rd.random_texts()[::10]
    assert len(texts) == 200
    for i, text in enumerate(texts):
        assert dev_line(dev, text) == rd.host_line(text), text
        for chunk in (63, 64, 65) + ((1,) if i % 10 == 0 else ()):
            want = rd.chunk_calls(lambda b, last: rd.host_line(b, last), text, chunk)
            got = rd.chunk_calls(lambda b, last: dev_line(dev, b, last, arrays=False), text, chunk)
            assert got == want, (text, chunk)


@pytest.mark.parametrize("tag", ["four_line", "wrapped_7", "mixed", "stray_plus", "every_qual_line_at", "err_qual_short", "fasta_wrapped", "tiny_reads"])
def test_max_reads(tag, dev):
    text, is_last, _, _ = rd.CORPUS[tag]
    whole = rd.parse_line(rd.host_line(text, is_last)[0])
    n = whole["nreads"] if whole.get("error") is None else 2          # err_qual_short: the second record is the bad one
    for is_last_ in (True, False):
        for m in sorted({1, n, max(n - 1, 1), n + 1}):
            assert dev_line(dev, text, is_last_, m) == rd.host_line(text, is_last_, m), (tag, m, is_last_)
    assert rd.host_line(rd.CORPUS["err_qual_short"][0], True, 1)[0].startswith("OK 1 ")      # an error behind the cut is not reached


def test_empty_text_and_device_view_only(dev):
    from smalt_amd import api
    assert dev_line(dev, b"") == rd.host_line(b"")
    assert dev_line(dev, b"", False) == rd.host_line(b"", False)
    text = rd.CORPUS["four_line"][0]
    hv, dv = dev.parse_raw(text, True, 0, host=False)
    assert hv is None and dv.nreads == 12 and dv.has_qual == 1 and dv.consumed == len(text)
    want = rd.parse_line(rd.host_line(text)[0])
    assert dev.readback(0)[0] == b"".join(want["reads"]) and dev.readback(1)[0] == b"".join(want["quals"])
    assert api.lib().smaltgpu_reads_parse_device(dev.h, text, len(text), 1, 0, None, None) == -3          # SMALTGPU_EARG: no view at all


def test_two_parses_on_one_handle(dev):
    """a long text, a short one, the long one again: the scratch of the earlier parse (marks, jump tables, record table) is stale
    and larger than what the later parse needs"""
    a, b = rd.CORPUS["tiny_reads"][0], rd.CORPUS["qual_prompt_lines"][0]
    first = dev_line(dev, a)
    assert first == rd.host_line(a)
    assert dev_line(dev, b) == rd.host_line(b)
    assert dev_line(dev, b"+x\nII\n") == rd.host_line(b"+x\nII\n")
    assert dev_line(dev, a) == first
    assert dev_line(dev, rd.CORPUS["fasta_wrapped"][0]) == rd.host_line(rd.CORPUS["fasta_wrapped"][0])


def _short_reads(nrec, drops):
    """nrec four-line FASTQ records with reads of 1 to 3 bases and no prompt character in a quality: two nodes a record.  drops:
    a '+' segment behind every record, which the chain of records passes through and drops (three nodes a record)"""
    out = []
    for i in range(nrec):
        n = 1 + i % 3
        out.append(b"@%x\n%s\n+\n%s\n" % (i, b"ACGTN"[i % 5:i % 5 + 1] * n, b"#5?I"[i % 4:i % 4 + 1] * n))
        if drops:
            out.append(b"+%x\nJJ\n" % i)
    return b"".join(out)


@pytest.mark.parametrize("drops", [False, True], ids=["records", "dropped_segments_between"])
def test_node_counts_at_the_borders_of_the_numbering_scan(drops, dev):
    """k_rd_sums and k_rd_number number the marked nodes RD_NODE_TILE (256) at a time, 64 to a wave: node counts of 2 and of one
    below, at and above two and four tiles (three and six with the dropped segments), records on both sides of every wave border"""
    for nrec in (1, 255, 256, 257, 513):
        text = _short_reads(nrec, drops)
        assert len(text) < 16_000
        want = rd.host_line(text)
        r = rd.parse_line(want[0])
        assert r["nreads"] == nrec and r["has_qual"] == 1 and [len(s) for s in r["reads"]] == [1 + i % 3 for i in range(nrec)]
        assert dev_line(dev, text) == want, (nrec, drops)


@pytest.mark.parametrize("groups", [0, 1], ids=["grid", "one_workgroup"])
def test_deep_chain(groups):
    """70 000 two-base reads whose quality lines begin with '@': three candidates a record, two of them on the chain, which is
    longer than 2^16 nodes; once over the whole grid, once with every pass over the prompts in one workgroup"""
    from smalt_amd import api
    text = rd.deep_text()
    levels = math.ceil(math.log2(3 * 70_000 + 1))
    assert levels > 16 and 2 * 70_000 > 1 << 16
    d = api.ReadsDevice(0)
    try:
        d.configure(0, groups, GUARD)
        line, used = dev_line(d, text)
        assert d.readback(2)[2] == 2 * levels + 7                    # launches: DESIGN "Reads parsed on the device"
        assert (line, used) == rd.host_line(text)
        assert rd.parse_line(line)["nreads"] == 70_000
    finally:
        d.close()


def test_mapping_straight_from_the_device_view(oracle_built, tmp_path):
    """the reads of a fixture parsed on the device and mapped from where they lie (map_batch_device) against map_batch on the reads
    the host parser returns"""
    from smalt_amd import api
    fx = gu.unpack([e for e in gu.MANIFEST_ALL if e["tag"] == "g_k11s4_cat"][0], tmp_path)
    text = gzip.open(os.path.join(gu.GOLD, "g_k11s4_cat.fq.gz"), "rb").read()
    want = rd.parse_line(rd.host_line(text, general=False)[0])
    assert want["nreads"] > 100 and want["has_qual"]
    gix = api.Index.load(fx["prefix"], 0)
    mp = api.Mapper(gix, want["nreads"], max(len(r) for r in want["reads"]))
    d = api.ReadsDevice(0)
    try:
        par = gix.default_params()
        exp_res, exp_stats = mp.map_batch(want["reads"], want["quals"], par)
        host, res_dev = d.parse(text)
        assert (host["names"], host["reads"], host["quals"]) == (want["names"], want["reads"], want["quals"])
        assert res_dev.nreads[0] == want["nreads"] and res_dev.read_off[0]
        mp.map_batch_device(res_dev.d_bases[0], res_dev.d_quals[0], res_dev.d_read_off[0], res_dev.nreads[0], res_dev.total_bases, par)
        res, stats = mp.unpack(mp.fetch_results())
        assert len(res) == want["nreads"]
        for i in range(want["nreads"]):
            assert res[i] == exp_res[i], i
        assert sum(len(r) for r in res) > want["nreads"] // 2
    finally:
        d.close()
        mp.close()
        gix.close()
