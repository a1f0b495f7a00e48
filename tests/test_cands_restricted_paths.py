"""The interval mode of the candidate stage (stage_cands_v2 in a restricted call of rmapPair) in the one-lane host build
(tests/hostemu with EMU_INTERVALS): the main-index cases of tests/test_gpu_cands_restricted.py against the oracle's dumps, text
for text.  Every case first asserts, from the predicates of tests/restricted_ref.py alone, that its inputs reach the branch it
is about -- this is where the inputs and the predicates are proven on a machine without a GPU, and what compiles the `#else`
halves of that code.  The fine-round case has no host build (its index is the kernel k_fine_index's); its predicates are checked
here against the oracle all the same."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import restricted_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu_bin():
    out = os.path.join(ROOT, "tests", "hostemu", "emu")
    tmp = "%s.%d.restricted" % (out, os.getpid())   # other workers build the same file at the same time: never run a half-written one
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", tmp, os.path.join(ROOT, "tests", "hostemu", "emu_main.cpp")], check=True)
    os.replace(tmp, out)
    return out


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle_built, tmp_path_factory):
    c = Ctx()
    c.seqs = rr.workload()
    c.cases = rr.cases(c.seqs)
    c.oix = ol.build_index(c.seqs, ["t%d" % i for i in range(len(c.seqs))], rr.K, rr.S)
    c.dir = tmp_path_factory.mktemp("restricted")
    c.pre = str(c.dir / "ix")
    assert ol.lib().or_index_write(c.oix, c.pre.encode()) == 0
    c.sop = np.ctypeslib.as_array(c.oix.contents.sop, shape=(len(c.seqs) + 1,)).copy()
    c.oracle = functools.lru_cache(maxsize=None)(lambda name: rr.oracle_case(ol, c.oix, c.cases[name]))
    yield c
    ol.lib().or_index_free(c.oix)


def _run_emu(emu_bin, ctx, name, **env_more):
    case = ctx.cases[name]
    fq, ivf = str(ctx.dir / (name + ".fq")), str(ctx.dir / (name + ".iv"))
    with open(fq, "wb") as f:
        for i, r in enumerate(case["reads"]):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    with open(ivf, "w") as f:
        for ivs in case["ivs"]:
            f.write(" ".join("%d %d %d" % v for v in ivs) + "\n")
    env = dict(os.environ, EMU_INTERVALS=ivf, EMU_STATS="1", **env_more)
    for v in ("EMU_WINDOW", "EMU_SPLIT", "EMU_CANDS", "EMU_CONCAT", "EMU_HISTORY"):
        env.pop(v, None)
    run = subprocess.run([emu_bin, "-H", str(case["ncut"]), ctx.pre, fq], check=True, capture_output=True, text=True, env=env)
    m = re.search(r"restricted: candcap (\d+), hcap_strand (\d+), lds_bytes (\d+)", run.stderr)
    assert m, run.stderr
    return run, tuple(int(x) for x in m.groups())


def _blocks(text):
    """dump text -> per read the compared lines"""
    out = []
    for ln in rr.stage_lines(text):
        if ln.startswith("READ "):
            out.append([])
        out[-1].append(ln)
    return out


CASES = [("geometry", {}), ("numbers", {}), ("counted", {}), ("direct", {"EMU_CANDCAP": "2048"}), ("halving", {}), ("many_keys", {}), ("long", {}),
         ("counted", {"EMU_LDS_BYTES": "64"}), ("halving", {"EMU_CANDCAP": "512"})]


@pytest.mark.parametrize("name,env", CASES, ids=[n + "".join("-" + k[4:].lower() + v for k, v in e.items()) for n, e in CASES])
def test_restricted_call_one_lane(name, env, emu_bin, ctx):
    """The same inputs under the slots the host build has by default and, where the environment says so, under slots small enough to
    move the strands to another branch: `counted` with a block of 64 bytes for LDS (all counts behind the ranking arrays),
    `halving` and `direct` with room for 512 and 2048 candidates (no room for the counts: the protocol searches the lists)."""
    case = ctx.cases[name]
    run, (candcap, hcap_strand, lds_bytes) = _run_emu(emu_bin, ctx, name, **env)
    exp = ctx.oracle(name)
    per = rr.strands_of(exp, case, ctx.sop, candcap, lds_bytes, long_inst=(name == "long"))
    sm = rr.summary([s for ss in per for s in ss])
    print(name, env, "candcap", candcap, "lds_bytes", lds_bytes, sm)
    if env.get("EMU_LDS_BYTES"):
        assert sm["counted_lds"] == 0 and sm["counted_sort"] >= 40
    elif name == "halving" and env:
        assert sm["direct"] >= 20 and sm["aborted"] >= 5 and sm["quirk"] >= 10
    else:
        rr.check_case(name, per, case)
    assert max(s.nkeys for ss in per for s in ss) <= hcap_strand
    got, want = _blocks(run.stdout), [rr.stage_lines(e[3]) for e in exp]
    assert len(got) == len(want)
    over = [i for i, ivs in enumerate(case["ivs"]) if len(ivs) > rr.IV_MAX]
    assert over == ([5] if name == "numbers" else [])
    for i, (a, b) in enumerate(zip(got, want)):
        if i in over:                                     # more than 2048 intervals: the read is refused, the others are not touched
            assert "emu: read %d: candidate stage -5" % i in run.stderr
            continue
        for j, (x, y) in enumerate(zip(a, b)):
            assert x == y, "read %d, line %d" % (i, j)
        assert len(a) == len(b), i
    assert ("emu:" in run.stderr) == bool(over), run.stderr
    if not over:                                          # nothing refused: the whole text, results included, hit lists apart
        strip = lambda t: [ln.rstrip() for ln in t.split("\n") if ln[:3] != "HL "]
        assert strip(run.stdout) == strip("".join(e[3] for e in exp))


def test_fine_round_inputs(ctx):
    """The fine-round case of the GPU test: the predicates hold (long form of the hit info, so no rank-to-offset order; the sum of
    the hit counts above the allocation; keys per strand below 200 k) with the geometry of a mapper for 100-base reads."""
    case = rr.fine_case(ctx.seqs)
    exp = rr.oracle_case(ol, ctx.oix, case, raw=True, fine=True)
    assert all(e[0] == 0 for e in exp)
    per = rr.strands_of(exp, case, ctx.sop, 131072, 20000)
    print(rr.check_case("fine", per, case))
    assert min(len(v) for v in case["ivs"][:6]) > 400
