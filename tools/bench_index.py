#!/usr/bin/env python3
"""Index construction: smaltgpu_index_build_device on a synthetic reference resident in HBM against
the reference's own single-threaded `smalt index` (oracle/_ref/smalt) on a bounded sample written to disk.
Prints one JSON line.  --fasta: the same reference written as a FASTA file and indexed from its text -- smaltgpu_index_build_text
(upload, parse and construction times) and the whole `smaltgpu-map index` program -- beside the same `smalt index` sample; the
result also goes to the file named by --out (default profiles/index_from_fasta.json).  --fastq: the same bases dressed as
four-line and as wrapped FASTQ records and indexed with SMALTGPU_TEXT_FASTQ, beside the FASTA text on its own route, with and
without the flag; one run over many short records for the share of the serial walk; `smalt index` on a FASTQ sample (default
--out profiles/index_from_fastq.json).  Not part of the bench.py contract."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_reference(ascii_ref, nsmp, k, s):
    """seconds the reference's `smalt index` takes for the first nsmp bases written as one FASTA sequence (None: it failed)"""
    smp = ascii_ref[:nsmp].cpu().numpy().tobytes()
    smalt = os.path.join(ROOT, "oracle", "_ref", "smalt")
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        fa = os.path.join(tmp, "s.fa")
        with open(fa, "wb") as f:
            f.write(b">chr1\n")
            for o in range(0, nsmp, 60):
                f.write(smp[o:o + 60] + b"\n")
        t = time.time()
        r = subprocess.run([smalt, "index", "-k", str(k), "-s", str(s), os.path.join(tmp, "s"), fa], capture_output=True)
        return time.time() - t if r.returncode == 0 else None


def fasta_mode(a, ref, ascii_ref, sop, names):
    """index from the text of a FASTA file: library call and whole program"""
    import hashlib
    from smalt_amd import api, synth
    tot = sop[-1]
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()  # noqa: E731
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        fa = os.path.join(tmp, "ref.fa")
        codes = ref.cpu().numpy()
        synth.write_fasta(fa, [codes[sop[i]:sop[i + 1]] for i in range(len(names))])
        t = time.time()
        text = open(fa, "rb").read()
        read_s = time.time() - t
        runs = []
        for _ in range(a.reps):
            t = time.time()
            ix = api.Index.from_fasta(text, a.k, a.s, 0)
            runs.append(dict(wall_ms=(time.time() - t) * 1e3, parse_ms=ix.parse_ms, build_ms=ix.build_ms))
            ix.close()
        _, _, times = api.parse_fasta(text, 0)                    # upload time and the share of each step
        want = os.path.join(tmp, "want")
        ix = api.Index.build_device(ascii_ref.data_ptr(), sop, names, a.k, a.s, 0)
        ix.save(want)
        ix.close()
        prog = []
        pre = os.path.join(tmp, "prog")
        for _ in range(a.reps):
            t = time.time()
            r = subprocess.run([os.path.join(ROOT, "smalt_amd", "smaltgpu-map"), "index", "-k", str(a.k), "-s", str(a.s), pre, fa], capture_output=True)
            prog.append(time.time() - t)
            assert r.returncode == 0, r.stderr.decode()[-2000:]
        same = md5(pre + ".sma") == md5(want + ".sma") and md5(pre + ".smi") == md5(want + ".smi")
        stderr_last = r.stderr.decode().strip().split("\n")
    nsmp = min(int(a.cpu_mbp * 1e6), tot)
    cpu_s = cpu_reference(ascii_ref, nsmp, a.k, a.s)
    best = min(runs, key=lambda x: x["wall_ms"])
    out = {"what": "index from the text of a FASTA file (smaltgpu_index_build_text, smaltgpu-map index)", "bases": tot, "text_bytes": len(text), "k": a.k, "s": a.s,
           "file_read_s": read_s, "library": {"runs": runs, "best": best, "upload_ms": times["upload_ms"], "parse_ms": times["parse_ms"],
                                              "parse_steps_ms": dict(zip(("block_summaries", "compose", "output_pass"), times["step_ms"])),
                                              "parse_text_GBps": len(text) / (times["parse_ms"] / 1e3) / 1e9},
           "program": {"wall_s": prog, "best_wall_s": min(prog), "bases_per_s": tot / min(prog), "files_equal_build_device": same, "progress": stderr_last},
           "cpu_reference": {"kind": "reference", "what": "`smalt index` (one thread, FASTA parse included)", "sample_bases": nsmp, "seconds": cpu_s,
                             "bases_per_s": (nsmp / cpu_s) if cpu_s else None},
           "program_speedup_per_base": (tot / min(prog)) / (nsmp / cpu_s) if cpu_s else None}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


def _wrap(a, width):
    """the bytes of `a` in lines of `width`"""
    n = len(a) // width * width
    body = np.concatenate([a[:n].reshape(-1, width), np.full((n // width, 1), 10, np.uint8)], axis=1).reshape(-1)
    return body if n == len(a) else np.concatenate([body, a[n:], np.array([10], np.uint8)])


def _lit(b):
    return np.frombuffer(b, dtype=np.uint8)


def fastq_texts(seqs, names, rng):
    """{dress: text}: FASTA wrapped at 60, four-line FASTQ, FASTQ wrapped at 60 with some quality lines beginning with '@'"""
    fa, four, wrapped = [], [], []
    for nm, sq in zip(names, seqs):
        q = rng.integers(35, 75, len(sq)).astype(np.uint8)
        q[0] = 73
        fa += [_lit(b">" + nm.encode() + b"\n"), _wrap(sq, 60)]
        four += [_lit(b"@" + nm.encode() + b"\n"), sq, _lit(b"\n+\n"), q, _lit(b"\n")]
        wrapped += [_lit(b"@" + nm.encode() + b"\n"), _wrap(sq, 60), _lit(b"+" + nm.encode() + b"\n"), _wrap(q, 60)]
    return {"fasta": np.concatenate(fa).tobytes(), "fastq_four_line": np.concatenate(four).tobytes(), "fastq_wrapped": np.concatenate(wrapped).tobytes()}


def short_records_text(nrec, length, rng):
    """nrec four-line FASTQ records of `length` bases, every row of the same width"""
    hd = np.frombuffer(b"".join(b"@r%08d\n" % i for i in range(nrec)), dtype=np.uint8).reshape(nrec, 11)
    sq = _lit(b"ACGT")[rng.integers(0, 4, (nrec, length))]
    q = rng.integers(35, 75, (nrec, length)).astype(np.uint8)
    q[:, 0] = 73
    nl = np.full((nrec, 1), 10, np.uint8)
    plus = np.tile(_lit(b"+\n"), (nrec, 1))
    return np.concatenate([hd, sq, nl, plus, q, nl], axis=1).tobytes()


def fastq_mode(a, ref, ascii_ref, sop, names):
    """index from FASTQ text: library call per dress, the walk's share on many short records, the reference on a sample"""
    import hashlib
    from smalt_amd import api
    tot = sop[-1]
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()  # noqa: E731
    rng = np.random.default_rng(20261021)
    host = ascii_ref.cpu().numpy()
    seqs = [host[sop[i]:sop[i + 1]] for i in range(len(names))]
    texts = fastq_texts(seqs, names, rng)
    steps = ("candidates_and_prefix_counts", "walk", "output_pass")
    out = {"what": "index from the text of a reference file with FASTQ records (smaltgpu_index_build_text_ex, SMALTGPU_TEXT_FASTQ)", "bases": tot, "k": a.k, "s": a.s, "dresses": {}}
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        want = os.path.join(tmp, "want")
        ix = api.Index.build_device(ascii_ref.data_ptr(), sop, names, a.k, a.s, 0)
        ix.save(want)
        ix.close()
        for dress, flag in (("fasta", False), ("fasta", True), ("fastq_four_line", True), ("fastq_wrapped", True)):
            text = texts[dress]
            runs, parses = [], []
            for rep in range(a.reps):
                t = time.time()
                ix = api.Index.from_fasta(text, a.k, a.s, 0, fastq=flag)
                runs.append(dict(wall_ms=(time.time() - t) * 1e3, parse_ms=ix.parse_ms, build_ms=ix.build_ms))
                if rep == 0:
                    got = os.path.join(tmp, "got")
                    ix.save(got)
                    same = md5(got + ".sma") == md5(want + ".sma") and md5(got + ".smi") == md5(want + ".smi")
                ix.close()
                _, _, times = api.parse_fasta(text, 0, fastq=flag)
                parses.append(dict(upload_ms=times["upload_ms"], parse_ms=times["parse_ms"], steps_ms=times["step_ms"]))
            route = "fasta" if dress == "fasta" else "fastq"
            best = min(parses, key=lambda x: x["parse_ms"])
            out["dresses"]["%s%s" % (dress, "_with_flag" if flag and dress == "fasta" else "")] = {
                "text_bytes": len(text), "route": route, "files_equal_build_device": same, "index_runs": runs, "parse_runs": parses, "best_parse_ms": best["parse_ms"],
                "best_parse_steps_ms": dict(zip(steps if route == "fastq" else ("block_summaries", "compose", "output_pass"), best["steps_ms"])),
                "parse_text_GBps": len(text) / (best["parse_ms"] / 1e3) / 1e9}
    del texts
    text = short_records_text(a.short_records, a.short_len, rng)
    parses = []
    for _ in range(a.reps):
        nm, sq, times = api.parse_fasta(text, 0, fastq=True)
        assert len(sq) == a.short_records and all(len(x) == a.short_len for x in sq[:1000])
        parses.append(dict(parse_ms=times["parse_ms"], steps_ms=times["step_ms"]))
    best = min(parses, key=lambda x: x["parse_ms"])
    out["short_records"] = {"records": a.short_records, "bases_per_record": a.short_len, "text_bytes": len(text), "parse_runs": parses, "best_parse_ms": best["parse_ms"],
                            "best_parse_steps_ms": dict(zip(steps, best["steps_ms"])), "walk_share": best["steps_ms"][1] / best["parse_ms"],
                            "walk_us_per_record": best["steps_ms"][1] * 1e3 / a.short_records}
    nsmp = min(int(a.cpu_mbp * 1e6), sop[1])
    smalt = os.path.join(ROOT, "oracle", "_ref", "smalt")
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        fa = os.path.join(tmp, "s.fq")
        with open(fa, "wb") as f:
            f.write(fastq_texts([host[:nsmp]], ["chr1"], rng)["fastq_wrapped"])
        t = time.time()
        r = subprocess.run([smalt, "index", "-k", str(a.k), "-s", str(a.s), os.path.join(tmp, "s"), fa], capture_output=True)
        cpu_s = time.time() - t if r.returncode == 0 else None
    out["cpu_reference"] = {"kind": "reference", "what": "`smalt index` (one thread) on wrapped FASTQ", "sample_bases": nsmp, "seconds": cpu_s, "bases_per_s": (nsmp / cpu_s) if cpu_s else None}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fasta", action="store_true", help="index from the text of a FASTA file (library call and `smaltgpu-map index`)")
    ap.add_argument("--fastq", action="store_true", help="index from FASTQ text with SMALTGPU_TEXT_FASTQ: four-line and wrapped records, many short records")
    ap.add_argument("--short-records", type=int, default=1_000_000, help="--fastq: records of the run that times the serial walk")
    ap.add_argument("--short-len", type=int, default=100, help="--fastq: bases per record of that run")
    ap.add_argument("--out", default=None, help="--fasta, --fastq: file the result is written to (default profiles/index_from_fasta.json, index_from_fastq.json)")
    ap.add_argument("--nchr", type=int, default=24)
    ap.add_argument("--chr-mbp", type=float, default=125.0)
    ap.add_argument("-k", type=int, default=13)
    ap.add_argument("-s", type=int, default=6)
    ap.add_argument("--cpu-mbp", type=float, default=100.0, help="size of the sample the CPU reference indexes")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "index_from_fastq.json" if a.fastq else "index_from_fasta.json")
    import torch
    from smalt_amd import api, gpuindex
    dev = torch.device("cuda", 0)
    chrlen = int(a.chr_mbp * 1e6)
    ref = gpuindex.make_reference_gpu(a.nchr, chrlen, 20261004, dev)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    ascii_ref = lut[ref.long()] if ref.numel() < (1 << 31) else torch.cat([lut[c.long()] for c in ref.split(1 << 28)])
    sop = [i * chrlen for i in range(a.nchr + 1)]
    names = ["chr%d" % (i + 1) for i in range(a.nchr)]
    tot = sop[-1]
    if a.fasta:
        return fasta_mode(a, ref, ascii_ref, sop, names)
    if a.fastq:
        return fastq_mode(a, ref, ascii_ref, sop, names)
    times = []
    info = None
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.time()
        ix = api.Index.build_device(ascii_ref.data_ptr(), sop, names, a.k, a.s, 0)
        wall = time.time() - t
        d = ix.info()
        info = dict(typ=int(d.typ), npos=int(d.npos), nwords=int(d.nwords))
        times.append((ix.build_ms, wall * 1e3))
        ix.close()
    dev_ms = min(t[0] for t in times)
    # the same image from the torch-op builder used by bench.py (setup plumbing), for scale
    torch.cuda.synchronize()
    t = time.time()
    try:
        idx, pos = gpuindex.build_perfect_index(ref, np.asarray(sop, dtype=np.int64), a.k, a.s)
        torch.cuda.synchronize()
        torch_ms = (time.time() - t) * 1e3
        del idx, pos
    except AssertionError:
        torch_ms = None
    # CPU reference on a bounded sample
    nsmp = int(a.cpu_mbp * 1e6)
    cpu_s = cpu_reference(ascii_ref, nsmp, a.k, a.s)
    ntup = (tot + a.s - 1) // a.s
    # algorithmic HBM bytes of the construction (PERFECT, 32-bit keys): every base read twice (packing, k-mer words) and
    # 0.4 B/base of packed words written; per sampled k-mer the (key, serial) pair written once (8 B) and read + written by
    # each of the ceil((2k+1)/8) radix passes (16 B per pass), the sorted keys read once more for the run ends (4 B); per
    # key the idx word written, read and written by the scan (12 B)
    passes = (2 * a.k + 1 + 7) // 8
    bytes_alg = tot * 2.4 + ntup * (8 + passes * 16 + 4) + (4 ** a.k) * 12
    out = {"what": "index construction, reference resident in HBM", "bases": tot, "k": a.k, "s": a.s, "index": info,
           "gpu_build_ms": dev_ms, "gpu_build_wall_ms": min(t[1] for t in times), "gpu_bases_per_s": tot / (dev_ms / 1e3),
           "torch_op_builder_ms": torch_ms,
           "roofline": {"bound": "hbm", "achieved": bytes_alg / (dev_ms / 1e3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                        "frac": bytes_alg / (dev_ms / 1e3) / 1e9 / 8000.0, "bytes_algorithmic": bytes_alg},
           "cpu_reference": {"kind": "reference", "what": "`smalt index` (one thread, FASTA parse included)", "sample_bases": nsmp,
                             "seconds": cpu_s, "bases_per_s": (nsmp / cpu_s) if cpu_s else None},
           "speedup_per_base": (tot / (dev_ms / 1e3)) / (nsmp / cpu_s) if cpu_s else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
