"""The FASTA reader in front of the index construction (`smaltgpu-map index`), without a GPU: the automaton of
smalt_amd/csrc/smg_fasta.hpp compiled for the host and run the way the kernels run it (tests/hostemu/fasta_check.cpp: block
summaries, their composition, the output pass), against what the reference's `smalt index -k 11 -s 2` made of the committed texts
(tests/golden/make_golden_fasta.py): names, lengths and -- through the oracle's index builder and writer -- the md5 of the
reference's `.sma` / `.smi` files.  Plus the new entry points of the C ABI and the usage text of the program."""
import ctypes
import os
import subprocess

import pytest

import fasta_data as fd
import golden_util as gu
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [64, 256, 0]                   # bytes of text per block; 0: the whole text in one block


@pytest.fixture(scope="session")
def fasta_check_bin():
    out = os.path.join(ROOT, "tests", "hostemu", "emu.fasta_check")
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", tmp, os.path.join(ROOT, "tests", "hostemu", "fasta_check.cpp")], check=True)
    os.replace(tmp, out)
    return out


def run_check(binary, text, block, tmp_path):
    p = tmp_path / "in.fa"
    p.write_bytes(text)
    r = subprocess.run([binary, str(p), str(block)], capture_output=True)
    lines = r.stdout.split(b"\n")
    if r.returncode:
        return r.returncode, lines[0].decode(), None, None
    n = int(lines[0].split()[1])
    names, seqs = [], []
    for ln in lines[1:1 + n]:
        nm, sq = ln.split(b" ")
        names.append("" if nm == b"-" else bytes.fromhex(nm.decode()).decode("latin-1"))
        seqs.append(b"" if sq == b"-" else sq)
    return 0, lines[0].decode(), names, seqs


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b256", "whole"])
@pytest.mark.parametrize("entry", fd.ACCEPTED, ids=[e["tag"] for e in fd.ACCEPTED])
def test_host_parse_gives_the_reference_index_files(entry, block, fasta_check_bin, oracle_built, tmp_path):
    rv, head, names, seqs = run_check(fasta_check_bin, fd.text_of(entry), block, tmp_path)
    assert rv == 0, head
    assert names == entry["names"]
    assert [len(s) for s in seqs] == entry["lengths"]
    oix = ol.build_index(seqs, [n.encode("latin-1") for n in names], entry["k"], entry["s"])
    pre = str(tmp_path / "ix")
    assert ol.lib().or_index_write(oix, pre.encode()) == 0
    ol.lib().or_index_free(oix)
    assert gu.md5(pre + ".sma") == entry["sma_md5"]
    assert gu.md5(pre + ".smi") == entry["smi_md5"]


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b256", "whole"])
@pytest.mark.parametrize("entry", fd.REFUSED, ids=[e["tag"] for e in fd.REFUSED])
def test_host_parse_reports_the_cause_of_a_refusal(entry, block, fasta_check_bin, tmp_path):
    rv, head, names, seqs = run_check(fasta_check_bin, fd.text_of(entry), block, tmp_path)
    if entry["expect"] == "short":          # the reader takes the text; the index construction refuses the sequence (as in the reference)
        assert rv == 0 and [len(s) for s in seqs] == [500, 333, 4]
        assert min(len(s) for s in seqs) < entry["k"]
    else:
        assert rv == 1 and head.startswith("REFUSED") and fd.CAUSE[entry["expect"]] in head, head


def test_host_parse_refuses_an_empty_text(fasta_check_bin, tmp_path):
    rv, head, _, _ = run_check(fasta_check_bin, b"", 64, tmp_path)
    assert rv == 1 and "empty" in head
    rv, head, _, _ = run_check(fasta_check_bin, b" \n\n\t\n", 64, tmp_path)
    assert rv == 1 and "no sequence" in head


@pytest.mark.parametrize("block", BLOCKS, ids=["b64", "b256", "whole"])
def test_host_parse_at_block_boundaries_equals_the_model(block, fasta_check_bin, tmp_path):
    """the texts of the GPU test, with a chosen byte on the last byte of a 64-byte block, and the Python statement of the automaton"""
    for tag, text in fd.boundary_texts(64).items():
        rv, head, names, seqs = run_check(fasta_check_bin, text, block, tmp_path)
        assert rv == 0, (tag, head)
        assert (names, seqs) == fd.parse_model(text), tag


def test_model_reads_the_committed_texts_as_the_reference_did():
    """the Python statement of the automaton (reference of the constructed GPU cases) against the reference's own reading"""
    for entry in fd.ACCEPTED:
        names, seqs = fd.parse_model(fd.text_of(entry))
        assert names == entry["names"] and [len(s) for s in seqs] == entry["lengths"], entry["tag"]


def test_new_abi_symbols_are_exported():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "smalt_amd", "csrc")], check=True)
    lib = ctypes.CDLL(os.path.join(ROOT, "smalt_amd", "libsmaltgpu.so"))
    hdr = open(os.path.join(ROOT, "include", "smaltgpu.h")).read()
    for name in ("smaltgpu_index_build_text", "smaltgpu_fasta_parse", "smaltgpu_fasta_free"):
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name


def test_index_subcommand_prints_its_usage():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "smalt_amd", "csrc")], check=True)
    r = subprocess.run([os.path.join(ROOT, "smalt_amd", "smaltgpu-map"), "index"], capture_output=True, text=True)
    assert r.returncode == 2
    assert "smaltgpu-map index" in r.stderr and "<reference.fa>" in r.stderr


def test_index_subcommand_checks_its_options(tmp_path):
    """-k 3 .. 20 and -s 1 .. 127 as the reference's menu (menu.c:595-596, :1272, :1281); a value that is no number is named"""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "smalt_amd", "csrc")], check=True)
    prog = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
    fa = tmp_path / "x.fa"
    fa.write_bytes(b">x\nACGTACGTACGTACGTACGT\n")
    for opts, word in ((["-k", "2"], "-k out of range"), (["-k", "21"], "-k out of range"), (["-s", "0"], "-s out of range"),
                       (["-s", "128"], "-s out of range"), (["-k", "x"], "not a number"), (["-s", "6b"], "not a number")):
        r = subprocess.run([prog, "index"] + opts + [str(tmp_path / "pre"), str(fa)], capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (opts, r.stderr)
        assert not os.path.exists(str(tmp_path / "pre.smi"))
    for args in (["-q", "1", str(tmp_path / "pre"), str(fa)], ["-k"], [str(fa)]):
        r = subprocess.run([prog, "index"] + args, capture_output=True, text=True)
        assert r.returncode == 2, args
