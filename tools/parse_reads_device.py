#!/usr/bin/env python
"""The parse of a block of reads alone, host against device: <n> reads of 150 bases as four-line FASTQ or as FASTA wrapped at 60
columns, parsed by smaltgpu_reads_parse (16 host threads and 1) and by smaltgpu_reads_parse_device (with the host view and without
it), <runs> times each after one warm-up call; one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python
tools/parse_reads_device.py fasta 262144 3 device` only the device route runs, for the per-kernel times.
usage: tools/parse_reads_device.py fastq|fasta [n = 262144] [runs = 3] [device]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smalt_amd import api  # noqa: E402


def make(kind, n, rlen=150):
    rng = np.random.default_rng(777)
    rd = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, rlen))]
    q = b"I" * rlen
    out = []
    for i in range(n):
        sq = rd[i].tobytes()
        if kind == "fastq":
            out.append(b"@r%d\n" % i + sq + b"\n+\n" + q + b"\n")
        else:
            out.append(b">r%d\n" % i + b"".join(sq[o:o + 60] + b"\n" for o in range(0, rlen, 60)))
    return b"".join(out)


def main():
    kind = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    only_device = len(sys.argv) > 4 and sys.argv[4] == "device"
    text = make(kind, n)
    L = api.lib()
    res = dict(kind=kind, reads=n, bytes=len(text), runs=runs)

    def timed(f):
        f()
        ms = []
        for _ in range(runs):
            t0 = time.perf_counter()
            f()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        return ms

    d = api.ReadsDevice(0)
    for host in (True, False):
        def dev():
            hv, dv = d.parse_raw(text, True, 0, host=host)
            assert dv.nreads == n
        res["device_ms_with_host_view" if host else "device_ms_device_view_only"] = timed(dev)
    res["launches"] = d.readback(2)[2]
    d.close()
    if not only_device:
        rs = L.smaltgpu_reads_create()
        for nt in (16, 1):
            def host_parse():
                v = api.ReadsView()
                assert L.smaltgpu_reads_parse(rs, text, len(text), 1, 0, nt, C.byref(v)) == 0 and v.nreads == n
            res["host_ms_%d_threads" % nt] = timed(host_parse)
        L.smaltgpu_reads_free(rs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
