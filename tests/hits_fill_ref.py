"""Plain restatement of the walk over the windows of stage_hits (smalt_amd/csrc/smg_cands.hpp, the strands of more keys than one
window) with the second, raised bound: numpy and Python integers only, no code shared with the library.  It is used to CHOOSE
inputs and to predict the number of windows; what the kernel writes is compared with the sorted run as ever (tests/hits_ref.py).

One window: every list offers a quota t = room * rest // remaining + 1 (room = W - lists); the safe bound is the least list
element just past such a quota, and every list gives those of its keys that lie below it.  When that leaves the window below
room * fill // 1024 keys, a second bound is put as far beyond the previous window's bound as the target lies beyond the count,
along the diagonal (the first window starts from the strand's least key); sequence by sequence it takes the sequence in which
its diagonal lies (never an earlier one than the safe bound's).  Every list's remaining keys below it are counted, and if they
fit the window (<= W) the second bound stands; if not, the safe one."""
import numpy as np

import hits_ref as hr

DIAGMASK = (1 << hr.KEY_DIAGBITS) - 1
FILL = 1024


class Window:
    """keys: keys of the window; safe: keys below the safe bound; last: the safe bound was ~0 (every list within its quota);
    tried: a second bound was counted; tot2: keys below it; raised: it stands; exhausted: lists with keys beyond the safe
    count that the second count used up; seq1, seq2: sequence of the safe bound and sequence in which the second bound's
    diagonal lies (the bound's own sequence, sequence by sequence)."""
    __slots__ = ("keys", "safe", "last", "tried", "tot2", "raised", "exhausted", "seq1", "seq2")


def seq_of(hx, pos):
    return int(np.searchsorted(hx.seqlo[:hx.nseq], pos, side="right")) - 1 if pos >= int(hx.seqlo[0]) else 0


def walk(e, W, hx, strand, seqbyseq, fill=FILL):
    """e: hits_ref.Expect of a strand with more than W keys; strand: 0 forward, 1 reverse -> [Window]"""
    lists = [np.sort(l >> np.uint64(hr.KEY_QBITS)).astype(np.int64) for l in e.lists]      # (sequence, diagonal); the read offset is constant in a list
    total = sum(l.size for l in lists)
    assert total > W > len(lists)
    room = W - len(lists)
    target = room * fill >> 10
    cur, remaining, out = [0] * len(lists), total, []
    dprev = min(int(l[0]) for l in lists) & DIAGMASK
    offs = 0 if strand else 1 << 32
    while remaining:
        w = Window()
        quota = [(room * (l.size - c)) // remaining + 1 for l, c in zip(lists, cur)]
        over = [int(l[c + t]) for l, c, t in zip(lists, cur, quota) if t < l.size - c]
        bound = min(over) if over else None
        cnt = [min(t, l.size - c) if bound is None else int(np.searchsorted(l[c:c + t], bound, side="left")) for l, c, t in zip(lists, cur, quota)]
        tot = sum(cnt)
        assert 0 < tot <= W
        w.safe, w.last, w.tried, w.raised, w.tot2, w.exhausted, w.seq1, w.seq2 = tot, bound is None, False, False, 0, 0, None, None
        if bound is not None and tot < target and (bound & DIAGMASK) > dprev:
            d2 = min(dprev + ((bound & DIAGMASK) - dprev) * target // tot, DIAGMASK)
            p2 = min(max(d2 - offs, 0), 0xFFFFFFFF)
            w.seq2 = seq_of(hx, p2)
            if seqbyseq:
                w.seq1 = bound >> hr.KEY_DIAGBITS
                w.seq2 = max(w.seq2, w.seq1)
                bound2 = (w.seq2 << hr.KEY_DIAGBITS) | d2
            else:
                w.seq1 = seq_of(hx, min(max((bound & DIAGMASK) - offs, 0), 0xFFFFFFFF))
                bound2 = d2
            if bound2 > bound:
                cnt2 = [int(np.searchsorted(l[c:], bound2, side="left")) for l, c in zip(lists, cur)]
                assert all(b >= a for a, b in zip(cnt, cnt2))
                w.tried, w.tot2 = True, sum(cnt2)
                if w.tot2 <= W:
                    w.raised = True
                    w.exhausted = sum(1 for l, c, a, b in zip(lists, cur, cnt, cnt2) if a < l.size - c == b)
                    cnt, tot, bound = cnt2, w.tot2, bound2
        if bound is not None:
            dprev = bound & DIAGMASK
        cur = [c + n for c, n in zip(cur, cnt)]
        remaining -= tot
        w.keys = tot
        out.append(w)
    return out
