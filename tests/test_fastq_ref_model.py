"""FASTQ-format reference files in front of the index construction, without a GPU: the Python walk over the records
(fastq_ref_data.parse_model_fq) against what the reference's `smalt index -k 11 -s 2` made of the committed texts
(tests/golden/make_golden_fastq_ref.py), and the rules of smalt_amd/csrc/smg_fastq_ref.hpp compiled for the host and run the way
the kernels run them (tests/hostemu/fastq_ref_check.cpp: block counts, granule prefixes, candidate list, the walk, the output pass)
against that model -- once more under the address and undefined-behaviour sanitizers, as a program of its own."""
import ctypes
import os
import subprocess

import pytest

import fasta_data as fd
import fastq_ref_data as fq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "fastq_ref_check.cpp")
BLOCKS = [64, 128, 256, 0]              # bytes of text per block; 0: the default


def _compile(name, flags):
    out = os.path.join(ROOT, "tests", "hostemu", name)
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-o", tmp, SRC], check=True)
    os.replace(tmp, out)
    return out


@pytest.fixture(scope="session")
def check_bin():
    return _compile("emu.fastq_ref_check", ["-O2"])


@pytest.fixture(scope="session")
def check_bin_san():
    return _compile("emu.fastq_ref_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run_check(binary, text, block, tmp_path):
    p = tmp_path / "in.fa"
    p.write_bytes(text)
    r = subprocess.run([binary, str(p), str(block)], capture_output=True)
    lines = r.stdout.split(b"\n")
    if r.returncode:
        return r.returncode, lines[0].decode("latin-1") + r.stderr.decode("latin-1")[-2000:], None, None
    n = int(lines[0].split()[1])
    names, seqs = [], []
    for ln in lines[1:1 + n]:
        nm, sq = ln.split(b" ")
        names.append("" if nm == b"-" else bytes.fromhex(nm.decode()).decode("latin-1"))
        seqs.append(b"" if sq == b"-" else sq)
    return 0, lines[0].decode(), names, seqs


def _model(text):
    try:
        return fq.parse_model_fq(text)
    except ValueError as e:
        assert fq.WRONG in str(e)
        return None


def _agrees(binary, text, block, tmp_path, what):
    want = _model(text)
    rv, head, names, seqs = run_check(binary, text, block, tmp_path)
    if want is None:
        assert rv == 1 and head.startswith("REFUSED") and fq.WRONG in head, (what, block, head)
    else:
        assert rv == 0, (what, block, head)
        assert (names, seqs) == want, (what, block)


def test_manifest_covers_the_shapes():
    tags = {e["tag"] for e in fq.MANIFEST}
    assert len(fq.ACCEPTED) >= 14 and len(fq.REFUSED) >= 4
    assert {"four_line", "wrapped", "qual_at_first", "plus_segment_between", "plus_segment_first", "fasta_then_fastq", "fasta_with_quality",
            "qual_at_behind_plus", "crlf_blank_noeol", "qual_one_more", "qual_extra_line", "qual_short_at_end", "qual_short_first",
            "header_after_header", "space_before_at", "space_before_at_in_fasta", "lower_iupac", "at_inside_fasta_data", "long_plus_header"} <= tags
    for e in fq.REFUSED:
        assert e["ref_message"] == [fq.WRONG], e["tag"]


@pytest.mark.parametrize("entry", fq.MANIFEST, ids=[e["tag"] for e in fq.MANIFEST])
def test_model_reads_the_committed_texts_as_the_reference_did(entry):
    got = _model(fq.text_of(entry))
    if entry["ref_status"]:
        assert got is None
    else:
        assert got is not None
        assert got[0] == entry["names"] and [len(s) for s in got[1]] == entry["lengths"]


def test_model_equals_the_fasta_model_on_fasta_texts():
    for entry in fd.ACCEPTED:
        text = fd.text_of(entry)
        assert fq.parse_model_fq(text) == fd.parse_model(text), entry["tag"]
    for text in fd.boundary_texts(64).values():
        assert fq.parse_model_fq(text) == fd.parse_model(text)


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b128", "b256", "default"])
@pytest.mark.parametrize("entry", fq.MANIFEST, ids=[e["tag"] for e in fq.MANIFEST])
def test_host_walk_agrees_with_the_model(entry, block, check_bin, tmp_path):
    _agrees(check_bin, fq.text_of(entry), block, tmp_path, entry["tag"])


def test_host_walk_names_the_refused_record(check_bin, tmp_path):
    entry = [e for e in fq.MANIFEST if e["tag"] == "qual_short_at_end"][0]
    text = fq.text_of(entry)
    rv, head, _, _ = run_check(check_bin, text, 64, tmp_path)
    at = text.index(b"@s3\n")
    assert rv == 1 and "'s3'" in head and "prompt 5 " in head and "byte %d)" % at in head and "397 characters for 401 bases" in head, head


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b128", "b256", "default"])
def test_host_walk_on_placed_and_plain_texts(block, check_bin, tmp_path):
    """chosen bytes on the first and the last byte of 64-byte blocks; FASTA texts take the same walk; texts the FASTA reader refuses"""
    for tag, text in fq.placed_texts(64).items():
        _agrees(check_bin, text, block, tmp_path, tag)
    for tag, text in fd.boundary_texts(64).items():
        _agrees(check_bin, text, block, tmp_path, tag)
    for entry in fd.MANIFEST:
        if entry["expect"] in ("ok", "fastq", "short"):
            _agrees(check_bin, fd.text_of(entry), block, tmp_path, entry["tag"])
    rv, head, _, _ = run_check(check_bin, fd.text_of([e for e in fd.MANIFEST if e["tag"] == "nohead"][0]), block, tmp_path)
    assert rv == 1 and fd.CAUSE["nohead"] in head
    rv, head, _, _ = run_check(check_bin, b" \n\n\t\n", block, tmp_path)
    assert rv == 1 and "no sequence" in head
    rv, head, _, _ = run_check(check_bin, b"+only\nIIII\n+dropped\nJJJJ\n", block, tmp_path)
    assert rv == 1 and "no sequence" in head


def test_host_walk_on_a_larger_wrapped_text(check_bin, tmp_path):
    text, names, seqs = fq.wrapped_fastq(7, 30_000)
    for block in (4096, 0):
        rv, head, got_names, got_seqs = run_check(check_bin, text, block, tmp_path)
        assert rv == 0, head
        assert (got_names, got_seqs) == (names, seqs)


def test_host_walk_under_sanitizers(check_bin_san, tmp_path):
    """the same program built with -fsanitize=address,undefined, run on its own: every fixture and every placed text"""
    texts = [(e["tag"], fq.text_of(e)) for e in fq.MANIFEST] + sorted(fq.placed_texts(64).items()) + [("wrapped", fq.wrapped_fastq(7, 30_000)[0])]
    for tag, text in texts:
        for block in (64, 0):
            _agrees(check_bin_san, text, block, tmp_path, tag)


def test_ex_abi_symbols_are_exported():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "smalt_amd", "csrc")], check=True)
    lib = ctypes.CDLL(os.path.join(ROOT, "smalt_amd", "libsmaltgpu.so"))
    hdr = open(os.path.join(ROOT, "include", "smaltgpu.h")).read()
    assert "#define SMALTGPU_TEXT_FASTQ 1u" in hdr
    for name in ("smaltgpu_index_build_text_ex", "smaltgpu_fasta_parse_ex"):
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name


def test_index_usage_names_both_formats():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "smalt_amd", "csrc")], check=True)
    r = subprocess.run([os.path.join(ROOT, "smalt_amd", "smaltgpu-map"), "index"], capture_output=True, text=True)
    assert r.returncode == 2
    assert "FASTA or FASTQ format" in r.stderr
