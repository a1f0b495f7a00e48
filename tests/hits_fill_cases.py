"""Inputs of the tests of the raised window bound of stage_hits (tests/test_gpu_hits_fill.py on the kernel,
tests/test_hits_fill_emu.py on the one-lane host build): the repeat reads of the k=13 s=6 workload of test_gpu_hits.py and one
probe read, and -- from the restatement of the walk (tests/hits_fill_ref.py) alone -- what happens in the windows of their
strands of 600 to 4000 keys.  Every configuration names the events it must reach; they are asserted before any comparison.

Events of a window: raised (the second bound stands), overshoot (its count is above the window: the safe bound's counts
stand), exhausted (a raised window uses up a list that the safe count had not), last (the safe bound is ~0 on the strand's last
window), cross+ / cross- (the second bound's diagonal lies in a later sequence than the safe bound; taken / not taken), eqW and
W+1 (a second count of exactly W and of W + 1 keys).

Two fill targets (SMALTGPU_HITS_FILL, the host program's argument; in 1/1024 of a window's room).  At 768 a second count above the window
is rare: at windows of 256 keys the strand of probe read 1753 holds the only one among the inputs (it is of W + 1 keys).  At
1024, the default, the walk overshoots often, and the exact fit and W + 1 are reached at both windows."""
import functools

import hits_fill_ref as hf
import hits_ref as hr

K, S, TAB = 13, 6, 120
PROBE = 1753
KEYS_MIN, KEYS_MAX = 600, 4000
ALWAYS = {"raised", "exhausted", "last", "cross+"}
# (fill, window) -> events the strands of 600 to 4000 keys must reach, in both hit-list modes
REQUIRED = {(768, 256): ALWAYS | {"overshoot", "W+1"}, (768, 300): ALWAYS,
            (1024, 256): ALWAYS | {"overshoot", "cross-", "eqW", "W+1"}, (1024, 300): ALWAYS | {"overshoot", "cross-", "eqW", "W+1"}}
CONFIGS = [(fill, w, concat) for (fill, w) in sorted(REQUIRED) for concat in (False, True)]
CONFIG_IDS = ["fill%d-w%d-%s" % (f, w, "concat" if c else "seqbyseq") for f, w, c in CONFIGS]


@functools.lru_cache(maxsize=None)
def inputs():
    """-> (sequences, reads): the reference of test_gpu_hits.workload(), its 200 reads cut from the repeat family and the probe read"""
    import test_gpu_hits as tgh
    seqs, rb = tgh.workload()
    return seqs, rb[200:] + [tgh._probe_read(PROBE)]


def walks(exp, window, hx, seqbyseq, fill):
    """hits_ref.Expect per strand -> {rs: [hits_fill_ref.Window]} of the strands above one window, and the events reached by those
    of KEYS_MIN..KEYS_MAX keys"""
    out, events = {}, set()
    for rs, e in enumerate(exp):
        if e.mode != hr.HITRUN_SORTED or e.keys.size <= window:
            continue
        ws = hf.walk(e, window, hx, rs & 1, seqbyseq, fill)
        assert sum(w.keys for w in ws) == e.keys.size and max(w.keys for w in ws) <= window
        out[rs] = ws
        if not KEYS_MIN <= e.keys.size <= KEYS_MAX:
            continue
        for i, w in enumerate(ws):
            if w.raised:
                events.add("raised")
                if w.exhausted:
                    events.add("exhausted")
            if w.tried:
                if not w.raised:
                    events.add("overshoot")
                if w.seq2 > w.seq1:
                    events.add("cross+" if w.raised else "cross-")
                if w.tot2 == window:
                    events.add("eqW")
                if w.tot2 == window + 1:
                    events.add("W+1")
            if w.last and i == len(ws) - 1:
                events.add("last")
    return out, events


def check_windows(exp, window, hx, seqbyseq, fill, windows, raised):
    """The uniform assertions on the walk: the configuration's events are reached (from the restatement alone); the stage's own
    count of windows and of raised bounds equals the restatement's on every strand; over the strands of KEYS_MIN..KEYS_MAX keys
    the walk takes fewer windows than the one with safe bounds alone (hits_ref.window_counts).  -> (windows before, after)"""
    ws, events = walks(exp, window, hx, seqbyseq, fill)
    missing = REQUIRED[(fill, window)] - events
    assert not missing, "events the inputs do not reach: %r" % sorted(missing)
    assert "eqW" not in REQUIRED[(fill, window)] or any(w.tried and w.tot2 == window and w.raised for v in ws.values() for w in v)
    assert "W+1" not in REQUIRED[(fill, window)] or any(w.tried and w.tot2 == window + 1 and not w.raised for v in ws.values() for w in v)
    before = after = 0
    for rs, e in enumerate(exp):
        if rs in ws:
            assert (int(windows[rs]), int(raised[rs])) == (len(ws[rs]), sum(1 for w in ws[rs] if w.raised)), (rs, int(windows[rs]), int(raised[rs]), len(ws[rs]))
            if KEYS_MIN <= e.keys.size <= KEYS_MAX:
                before += len(hr.window_counts(e, window))
                after += len(ws[rs])
        else:
            assert int(windows[rs]) == 0 and int(raised[rs]) == 0, rs
    assert len(ws) >= 20 and after < before
    return before, after
