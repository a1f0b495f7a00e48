"""The read parser of smalt_amd/csrc/smg_reads_dev.hpp without a GPU: its rules compiled for the host and run the way the kernels
run them (tests/hostemu/reads_dev_check.cpp: block counts, granule prefixes, candidates, the speculative step for every node, the
jump tables, the marking, the numbering in tiles, the output pass per block and lane) against smaltgpu_reads_parse, which is host
code and is called through ctypes (reads_dev_data.host_line) -- on the corpus of tests/reads_dev_data.py, on 2000 random texts
whole and cut in two at every byte offset, and once more under the address and undefined-behaviour sanitizers, as a program of
its own."""
import os
import subprocess

import pytest

import reads_dev_data as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "reads_dev_check.cpp")
BLOCKS = [64, 4096, rd.BLOCK, 0]       # bytes of text per block; 0: the default


def _compile(name, flags):
    out = os.path.join(ROOT, "tests", "hostemu", name)
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-o", tmp, SRC], check=True)
    os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def lib_built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "smalt_amd", "csrc")], check=True)


@pytest.fixture(scope="module")
def check_bin():
    return _compile("emu.reads_dev_check", ["-O2"])


@pytest.fixture(scope="module")
def check_bin_san():
    return _compile("emu.reads_dev_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run_check(binary, cases, block, tmp_path):
    """cases: case records -> the lines the program printed"""
    p = tmp_path / "cases.bin"
    p.write_bytes(b"".join(cases))
    r = subprocess.run([binary, str(p), str(block)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode("latin-1")[-3000:]
    return r.stdout.decode("latin-1").split("\n")[:-1]


def test_abi_symbols_and_usage(lib_built):
    from smalt_amd import api
    hdr = open(os.path.join(ROOT, "include", "smaltgpu.h")).read()
    for name in ("smaltgpu_reads_dev_create", "smaltgpu_reads_dev_free", "smaltgpu_reads_parse_device", "smaltgpu_reads_dev_configure", "smaltgpu_reads_dev_readback"):
        assert name + "(" in hdr, name
        assert hasattr(api.lib(), name), name
    assert "smaltgpu_reads_device_view" in hdr and hasattr(api, "ReadsDevice") and hasattr(api, "ReadsDeviceView")
    r = subprocess.run([os.path.join(ROOT, "smalt_amd", "smaltgpu-map")], capture_output=True, text=True)
    assert r.returncode == 2 and "SMALTGPU_DEVICE_PARSE=1" in r.stderr


@pytest.mark.parametrize("tag", sorted(rd.CORPUS), ids=sorted(rd.CORPUS))
def test_corpus_cases_exercise_their_rule(tag, lib_built):
    rd.check_case(tag)


def test_corpus_covers_the_shapes(lib_built):
    tags = set(rd.CORPUS)
    assert {"four_line", "wrapped_7", "wrapped_60", "fasta_wrapped", "fasta_one_line", "mixed", "crlf", "blank_lines", "no_final_newline", "letters", "header_no_name",
            "header_words", "empty_read", "qual_prompt_lines", "every_qual_line_at", "stray_plus", "err_noprompt", "err_qual_short", "err_qual_long", "err_qual_short_at_end",
            "tiny_reads", "header_ends_text", "plus_ends_text"} <= tags
    assert sum(t.startswith("placed_") for t in tags) == 36
    # the four-line path of the host parser and its general rules agree on every whole text of the corpus but the two that end in a
    # record of fewer than four lines: there the four-line path leaves the last record, and the device parser follows the general rules
    for tag, (text, is_last, _, _) in rd.CORPUS.items():
        same = rd.host_line(text, is_last, general=False) == rd.host_line(text, is_last)
        assert same == (tag not in ("header_ends_text", "plus_ends_text")), tag
    n = 2 * rd.REC_PER_TILE // 3
    assert rd.parse_line(rd.host_line(rd.CORPUS["tiny_reads"][0])[0])["nreads"] == n and len(rd.CORPUS["tiny_reads"][0]) / n < 10      # > 400 records begin in a tile


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b4096", "b8192", "default"])
def test_host_build_on_the_corpus(block, check_bin, lib_built, tmp_path):
    tags = sorted(rd.CORPUS)
    got = run_check(check_bin, [rd.case_record(rd.CORPUS[t][0], 0, rd.CORPUS[t][1]) for t in tags], block, tmp_path)
    assert len(got) == len(tags)
    for t, g in zip(tags, got):
        assert g == rd.host_line(rd.CORPUS[t][0], rd.CORPUS[t][1])[0], (t, block)
    # max_reads at 1, one below the number of records and at it, as a chunk and as the last text
    cases, want = [], []
    for t in tags:
        text = rd.CORPUS[t][0]
        n = rd.parse_line(rd.host_line(text)[0]).get("nreads") or 2
        for last in (True, False):
            for m in sorted({1, max(n - 1, 1), n}):
                cases.append(rd.case_record(text, 0, last, m))
                want.append(rd.host_line(text, last, m)[0])
    assert run_check(check_bin, cases, block, tmp_path) == want


def test_host_build_on_the_corpus_cut_at_every_offset(check_bin, lib_built, tmp_path):
    """the texts of up to 300 bytes: text[0, c) as a chunk, then the rest from `consumed` as the last text"""
    tags = [t for t in sorted(rd.CORPUS) if len(rd.CORPUS[t][0]) <= 300]
    assert len(tags) >= 20
    got = run_check(check_bin, [rd.case_record(rd.CORPUS[t][0], 1) for t in tags], 64, tmp_path)
    k = 0
    for t in tags:
        text = rd.CORPUS[t][0]
        for c in range(1, len(text)):
            want, used = rd.host_line(text[:c], False)
            assert got[k] == want, (t, c)
            assert got[k + 1] == rd.host_line(text[used:], True)[0], (t, c)
            k += 2
    assert k == len(got)


def test_host_build_on_random_texts(check_bin, lib_built, tmp_path):
    """2000 seeded texts of up to 200 bytes over @ + > \\n \\r space A c N I: whole, whole with max_reads = 2, and cut in two at every
    byte offset (the first part with is_last = 0, the rest from where it stopped); views, consumed, error code and message"""
    texts = rd.random_texts()
    assert len(texts) == 2000 and max(len(t) for t in texts) <= 200
    got = run_check(check_bin, [rd.case_record(t) for t in texts] + [rd.case_record(t, 0, True, 2) for t in texts] + [rd.case_record(t, 1) for t in texts], 64, tmp_path)
    k, kinds = 0, {"ERR " + rd.E_NOPROMPT: 0, "ERR sequence and": 0, "OK 0": 0, "OK": 0}
    for m in (0, 2):
        for t in texts:
            want = rd.host_line(t, True, m)[0]
            assert got[k] == want, (t, m)
            k += 1
            for key in kinds:
                if want.startswith(key):
                    kinds[key] += 1
                    break
    assert all(v > 50 for v in kinds.values()), kinds              # the texts reach both errors, no read and reads
    for t in texts:
        for c in range(1, len(t)):
            want, used = rd.host_line(t[:c], False)
            assert got[k] == want, (t, c)
            assert got[k + 1] == rd.host_line(t[used:], True)[0], (t, c)
            k += 2
    assert k == len(got)


def test_host_build_on_the_deep_chain(check_bin, lib_built, tmp_path):
    text = rd.deep_text()
    got = run_check(check_bin, [rd.case_record(text)], 0, tmp_path)
    assert got == [rd.host_line(text)[0]] and got[0].startswith("OK 70000 1 ")


def test_host_build_under_sanitizers(check_bin_san, lib_built, tmp_path):
    """the same program built with -fsanitize=address,undefined, run on its own over the corpus: every text in a buffer of its own
    size, whole, and the short ones cut at every offset"""
    tags = sorted(rd.CORPUS)
    for block in (64, 0):
        got = run_check(check_bin_san, [rd.case_record(rd.CORPUS[t][0], 0, rd.CORPUS[t][1]) for t in tags], block, tmp_path)
        assert got == [rd.host_line(rd.CORPUS[t][0], rd.CORPUS[t][1])[0] for t in tags]
    short = [t for t in tags if len(rd.CORPUS[t][0]) <= 100]
    got = run_check(check_bin_san, [rd.case_record(rd.CORPUS[t][0], 1) for t in short], 64, tmp_path)
    assert len(got) == sum(2 * (len(rd.CORPUS[t][0]) - 1) for t in short) and not any(g.startswith("ERR the") for g in got)
