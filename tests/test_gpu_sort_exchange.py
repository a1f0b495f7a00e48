"""The cross-lane exchanges of the register sorts (keep_side_u64 in smg_exec.h) through smaltgpu_sort_u64_batch, forms 0-5,
against np.sort.  An exchange decides with one compare, o < v, turned round in the upper lane; that is the network only because
equal keys make the choice immaterial and because the ~0 beyond n is just another equal key.  So the arrays here put equal keys,
and keys one bit apart, on the two ends of comparators: every comparator of the network pairs the logical element i with
i ^ x, x = j for a half-cleaner and x = k - 1 for the mirror step of a merge, and an array is built per x with a[i] and
a[i ^ x] made a pair.  Which array position holds which logical element differs by form (`_layout`), and the arrays are laid out
so that the pairs are pairs of the network's own elements.  The wrapper puts a guard array behind the last array of every
launch and raises when it does not come back as it went in."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL = np.uint64(0xFFFFFFFFFFFFFFFF)
# form -> (largest array, keys per lane E of the register layout or 0, layouts of the arrays)
#   "reg":   the register forms and a chunk of the chunked sort load position 64 r + l into register r of lane l and treat it as
#            logical element E l + r (E = 4, 8, 16; the chunked sort: E = 16 in every chunk of 1024 keys)
#   "plain": position = logical element (the network in LDS or in memory, the chunked sort's merges j = 512 .. 1 and above)
FORMS = {0: (256, 4, ["reg"]), 1: (512, 8, ["reg"]), 2: (1024, 16, ["reg"]), 3: (1024, 0, ["plain"]), 4: (65536, 0, ["plain"]),
         5: (65536, 16, ["plain", "reg"])}
FORM_IDS = ["reg4", "reg8", "reg16", "lds", "hbm", "chunked"]
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024]
LENGTHS_HBM = [1025, 2047, 2048, 2049, 16384 + 1]
PALETTES = [2, 3, 4]
ONE_BIT = ["bit0", "bit31", "bit32", "bit63", "high", "low"]


@pytest.fixture(scope="module")
def sort_mapper():
    """The sorts take a mapper for its device and stream only: any small index will do."""
    from smalt_amd import api, synth
    ch = synth.make_reference(1, 20_000, seed=5, repeat_frac=0.0)
    gix = api.Index.build([synth.codes_to_ascii(c) for c in ch], ["c0"], 13, 6, 0)
    mp = api.Mapper(gix, 8, 100)
    yield mp
    mp.close()
    gix.close()


def _padded(form, n):
    """Size of the network that sorts n keys in this form: the register forms always run all of it, the others the next power of
    two; at least a chunk, so that one pattern serves the chunked sort's layout too."""
    nmax, e, _ = FORMS[form]
    if form <= 2:
        return nmax
    np2 = 1024
    while np2 < n:
        np2 *= 2
    return np2


def _masks(size, n):
    """x of every comparator distance of a network of `size` elements: j = 1 .. size / 2 and k - 1 = 1 .. size - 1.  Above 2049
    keys only those that the smaller arrays cannot reach: the chunked sort's cross-lane steps (j below 64, in both layouts), the
    last mirror step inside a chunk and everything that spans chunks."""
    t = int(size).bit_length() - 1
    xs = sorted(set([1 << u for u in range(t)] + [(1 << u) - 1 for u in range(1, t + 1)]))
    if n > 2049:
        xs = [x for x in xs if x in (1, 2, 4, 8, 16, 32, 1023) or x >= 1024]
    return xs


def _layout(val, kind, e):
    """Logical elements -> array positions."""
    if kind == "plain":
        return val
    c = 64 * e
    p = np.arange(val.size)
    q = p & (c - 1)
    return val[(p - q) + e * (q % 64) + q // 64]


def _pair_values(size, x, variant, rng):
    """`size` logical elements in which i and i ^ x form a pair."""
    i = np.arange(size)
    t = np.minimum(i, i ^ x)                                   # the pair's name
    first = i == t
    rnd = rng.integers(0, 1 << 63, size=size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=size, dtype=np.uint64)
    if isinstance(variant, int):                               # so many distinct values, both ends of a pair equal
        palette = np.sort(rnd[:variant])
        if variant == 2:
            palette[1] = FULL                                  # one of them the padding's own value
        return palette[rng.integers(0, variant, size=size)][t]
    if variant.startswith("bit"):                              # the rest random but equal within the pair
        bit = np.uint64(1) << np.uint64(int(variant[3:]))
        coin = rng.integers(0, 2, size=size).astype(bool)[t]
        return (rnd[t] & ~bit) | np.where(first == coin, bit, np.uint64(0))
    lo32 = np.uint64(0xFFFFFFFF)
    if variant == "high":                                      # low words equal within the pair
        return (rnd & ~lo32) | (rnd[t] & lo32)
    assert variant == "low"
    return (rnd[t] & ~lo32) | (rnd & lo32)


def _cases(form, n, variants, rng):
    """Every distance x layout x variant at length n -> (label, array) list"""
    _, e, layouts = FORMS[form]
    size = _padded(form, n)
    out = []
    for x in _masks(size, n):
        for kind in layouts:
            if kind == "reg" and form == 5 and x >= 1024:
                continue                                       # (the layouts agree on the chunk an element is in)
            for v in variants:
                out.append(((n, x, kind, v), _layout(_pair_values(size, x, v, rng), kind, e)[:n].copy()))
    return out


def _sort_and_compare(mp, form, cases):
    assert cases
    out = mp.sort_u64_batch([a for _, a in cases], form)        # (raises when the guard behind the last array was written)
    assert len(out) == len(cases)
    for (label, a), o in zip(cases, out):
        assert o.dtype == np.uint64 and np.array_equal(o, np.sort(a)), (form, label)


def _sizes(form):
    """The form's largest network of at most 1024 keys; for the sorts in memory also 4096 keys: chunks, the mirror step and a
    half-cleaner across chunks, and the chunked sort's register passes j = 512 .. 1."""
    return [min(FORMS[form][0], 1024)] + ([4096] if form >= 4 else [])


@pytest.mark.parametrize("form", range(6), ids=FORM_IDS)
def test_equal_keys_on_both_ends_of_a_comparator(sort_mapper, form):
    """a[i] == a[partner(i)] for all i, for every distance of the form: arrays of 2 (one of them ~0), 3 and 4 distinct values;
    and all keys equal."""
    rng = np.random.default_rng(300 + form)
    cases = []
    for n in _sizes(form):
        cases += _cases(form, n, PALETTES, rng)
        cases += [((n, 0, "equal", v), np.full(n, v, dtype=np.uint64)) for v in (0, 0x0000000100000000, 0x00000000FFFFFFFF, int(FULL))]
    for _, a in cases:
        assert np.unique(a).size <= 4
    _sort_and_compare(sort_mapper, form, cases)


@pytest.mark.parametrize("form", range(6), ids=FORM_IDS)
def test_pairs_one_bit_apart(sort_mapper, form):
    """The two ends of a comparator differ in bit 0, 31, 32 or 63 only, in the high word only, in the low word only: a compare
    that looked at one half of the key, or took the halves in the wrong order or as signed numbers, orders some pair wrongly."""
    rng = np.random.default_rng(310 + form)
    cases = []
    for n in _sizes(form):
        cases += _cases(form, n, ONE_BIT, rng)
    _sort_and_compare(sort_mapper, form, cases)


@pytest.mark.parametrize("form", range(6), ids=FORM_IDS)
def test_lengths(sort_mapper, form):
    """Every length of the issue that the form admits, the contents of the two tests above cut off at n: the keys beyond n are
    the ~0 padding (register forms) or comparators that are never visited (the networks in memory)."""
    rng = np.random.default_rng(320 + form)
    lengths = [n for n in LENGTHS + (LENGTHS_HBM if form >= 4 else []) if n <= FORMS[form][0]]
    assert lengths[-1] == (FORMS[form][0] if form <= 3 else 16385)
    cases = []
    for n in lengths:
        cases += _cases(form, n, [3, "bit0", "bit32", "bit63"] if n > 2049 else PALETTES + ONE_BIT, rng)
    _sort_and_compare(sort_mapper, form, cases)


@pytest.mark.parametrize("form", range(6), ids=FORM_IDS)
def test_full_keys_beside_the_padding(sort_mapper, form):
    """Real keys equal to ~0 next to the padding: n = 1000 of 1024 slots (250 of 256 and 500 of 512 in the smaller register
    forms).  All keys ~0; a random third; the last 40; and, per distance, exactly the keys whose partner lies beyond n."""
    rng = np.random.default_rng(330 + form)
    _, e, layouts = FORMS[form]
    size = min(FORMS[form][0], 1024)
    n = size * 1000 // 1024
    rnd = lambda: rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    a1, a2 = rnd(), rnd()
    a1[rng.integers(0, 3, size=n) == 0] = FULL
    a2[-40:] = FULL
    cases = [((n, 0, "all", 0), np.full(n, FULL, dtype=np.uint64)), ((n, 0, "third", 0), a1), ((n, 0, "tail", 0), a2)]
    pos = _layout(np.arange(size), "plain", e)
    for x in _masks(size, n):
        for kind in layouts:
            where = _layout(np.arange(size), kind, e)          # position -> logical element
            at = np.empty(size, dtype=np.int64)
            at[where] = pos                                    # logical element -> position
            partner_beyond = at[where ^ x] >= n
            a = rnd()
            a[partner_beyond[:n]] = FULL
            cases.append(((n, x, kind, "partner"), a))
    _sort_and_compare(sort_mapper, form, cases)
