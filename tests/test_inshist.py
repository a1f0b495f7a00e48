"""Insert-size histograms (smalt_amd/csrc/smg_inshist.cpp) against files of the reference program, through ctypes on
libsmaltgpu.so; host code, no GPU.  tests/golden/inshist_<tag>.sample.txt is the tail of a `smalt sample -o` file,
inshist_<tag>.stdout.txt what `smalt map -g` printed after reading that file back (tests/golden/make_golden_inshist.py):
`all` has bins of width 1, `first` (100 pairs) wider ones.  Reading, writing, the smoothing arithmetic (the smoothed print is
made from the counts the reader smoothed), the reader's errors and the sampling interval."""
import os

import pytest

import golden_util as gu

TAGS = ["all", "first"]


def _fixture(tag, ext):
    return open(os.path.join(gu.GOLD, "inshist_%s.%s.txt" % (tag, ext)), "rb").read()


@pytest.fixture(scope="module")
def api():
    from smalt_amd import api
    api.lib()
    return api


@pytest.fixture(scope="module")
def sample_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("inshist")
    paths = {}
    for tag in TAGS:
        paths[tag] = str(d / (tag + ".smp"))
        with open(paths[tag], "wb") as f:
            # the reader skips what stands ahead of the section: SAM lines and the prints
            f.write(b"p0\t77\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n" + _fixture(tag, "sample"))
    return paths


def _header(text):
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in text.decode().split("\n") if ln.startswith("HISTO_") and " " in ln}


def test_fixtures_cover_both_bin_widths():
    assert _header(_fixture("all", "sample"))["HISTO_SCALFAC"] == [1]
    assert _header(_fixture("first", "sample"))["HISTO_SCALFAC"][0] > 1


@pytest.mark.parametrize("tag", TAGS)
def test_section_read_and_written_back(api, sample_files, tag):
    h = api.InsertHistogram.read(sample_files[tag])
    want = _fixture(tag, "sample")
    assert h.text(api.HIST_SECTION) == want[want.index(b"# SMALT histogram of insert sizes\n"):]
    hd = _header(want)
    assert h.bounds() == (hd["HISTO_INSIZLO"][0], hd["HISTO_INSIZHI"][0], hd["HISTO_BINNUM"][0], hd["HISTO_TOTNUM"][0])
    h.close()


@pytest.mark.parametrize("tag", TAGS)
def test_prints_after_reading_are_the_reference_programs(api, sample_files, tag):
    """the sampled and the smoothed print at 80 columns, byte for byte what `smalt map -g` wrote: pins bandwidth, kernel and window"""
    h = api.InsertHistogram.read(sample_files[tag])
    assert h.text(api.HIST_SAMPLED, 80) + h.text(api.HIST_SMOOTHED, 80) == _fixture(tag, "stdout")
    # `smalt sample` printed the same histogram (made from the sample, smoothed once) ahead of the section
    want = _fixture(tag, "sample")
    assert b"# Sampled histogram\n" + h.text(api.HIST_SAMPLED, 80) + b"# Smoothed histogram\n" + h.text(api.HIST_SMOOTHED, 80) == want[:want.index(b"# SMALT histogram")]
    h.close()


@pytest.mark.parametrize("tag", TAGS)
def test_counts_and_cumulative_counts(api, sample_files, tag):
    h = api.InsertHistogram.read(sample_files[tag])
    want = _fixture(tag, "sample")
    hd = _header(want)
    lo, hi, width = hd["HISTO_INSIZLO"][0], hd["HISTO_INSIZHI"][0], hd["HISTO_SCALFAC"][0]
    body = want[want.index(b"HISTO_QUARTILES"):].decode().split("\n")[1:]
    bins = [int(ln.split()[1]) for ln in body if ln and not ln.startswith("HISTO_END")]
    assert len(bins) == hd["HISTO_BINNUM"][0]
    run = 0
    for b, c in enumerate(bins):
        run += c
        for size in {lo + b * width, min(hi, lo + b * width + width - 1)}:
            assert h.count(size, smoothed=False) == (c, run), size
    assert h.count(lo - 1, smoothed=False) == (0, 0) and h.count(hi + 1, smoothed=True) == (0, 0)
    # the smoothed counts are whole numbers of a window that never gains mass
    sm = [h.count(lo + b * width, smoothed=True)[0] for b in range(len(bins))]
    assert all(x >= 0 for x in sm) and 0 < sum(sm) <= sum(bins)
    assert h.count(hi, smoothed=True)[1] == sum(sm)
    h.close()


def _broken(tag, how):
    lines = _fixture(tag, "sample").decode().split("\n")
    first_bin = next(i for i, ln in enumerate(lines) if ln.startswith("HISTO_QUARTILES")) + 1
    if how == "no_end":
        lines = [ln for ln in lines if not ln.startswith("HISTO_END")]
    elif how == "totnum":
        lines = [("HISTO_TOTNUM %d" % (int(ln.split()[1]) + 1)) if ln.startswith("HISTO_TOTNUM") else ln for ln in lines]
    elif how == "shifted_bin":
        size, count = lines[first_bin + 3].split()
        lines[first_bin + 3] = "%d %s" % (int(size) + 1, count)
    elif how == "extra_bin":
        end = lines.index("HISTO_END")
        width = _header(_fixture(tag, "sample"))["HISTO_SCALFAC"][0]
        lines.insert(end, "%d 0" % (int(lines[end - 1].split()[0]) + width))
    return "\n".join(lines).encode()


@pytest.mark.parametrize("how", ["no_end", "totnum", "shifted_bin", "extra_bin"])
@pytest.mark.parametrize("tag", TAGS)
def test_broken_files_are_errors(api, tmp_path, tag, how):
    text = _broken(tag, how)
    assert text != _fixture(tag, "sample")
    p = str(tmp_path / "broken.smp")
    open(p, "wb").write(text)
    with pytest.raises(api.SmaltGpuError):
        api.InsertHistogram.read(p)
    with pytest.raises(api.SmaltGpuError):
        api.InsertHistogram.read(str(tmp_path / "no_such_file"))


@pytest.mark.parametrize("npairs,every,interval", [(1800, 100, 1), (21600, 100, 5), (21600, 3, 3), (500000, 100, 100), (500000, 0, 122)])
def test_sampling_interval(api, npairs, every, interval):
    assert api.sample_interval(npairs, every) == interval


def test_histogram_from_a_sample(api):
    """bins from a sample (quartiles of the sorted sample, six inter-quartile ranges, 3 * sqrt(n) bins of whole width): values worked
    out by hand.  101 sizes 250 .. 350: median 300, quartiles 275 / 325, range 300, 3 * sqrt(101) = 30 bins of width 10 from 150"""
    h = api.InsertHistogram.from_sample(list(range(350, 249, -1)))
    assert h.bounds() == (150, 449, 30, 101)
    head = h.text(api.HIST_SECTION).decode().split("\n")
    assert head[:8] == ["# SMALT histogram of insert sizes", "HISTO_START", "HISTO_BINNUM 30", "HISTO_SCALFAC 10", "HISTO_INSIZLO 150", "HISTO_INSIZHI 449",
                        "HISTO_TOTNUM 101", "HISTO_QUARTILES 275 300 325"]
    assert h.count(250, smoothed=False) == (10, 10) and h.count(350, smoothed=False) == (1, 101) and h.count(249, smoothed=False) == (0, 0)
    h.close()
    # few bins: a sample with equal quartiles has no range and gives no histogram
    with pytest.raises(api.SmaltGpuError):
        api.InsertHistogram.from_sample([300] * 50)
    # a narrow sample: the range (6 x 2 = 12) is below the 16 bins of the minimum, so there is a bin of width 1 per size
    h = api.InsertHistogram.from_sample([298, 299, 300, 301, 302] * 8)
    assert h.bounds() == (300 - 6, 300 + 5, 12, 40)
    h.close()


def _smoothed_by_the_rule(bins):
    """DESIGN.md 5e in plain Python: bandwidth from the binned inter-quartile range, weights exp(-x^2 / 2) / sqrt(2 pi) out to three
    bandwidths, the window [b - reach, b + reach) with the weights counted from the bin's own number below `reach` (zeros behind
    the last weight), sums truncated"""
    import math
    n, total = len(bins), sum(bins)
    run, mark, at = 0, total // 4, []
    for b, c in enumerate(bins):
        if len(at) == 3:
            break
        run += c
        if run > mark:
            at.append(b)
            run -= c // 2
            mark = total * len(at) // 4
    iqr = at[2] - at[0] if len(at) == 3 and n > 3 else 0
    bw = max(3, int(0.9 * math.pow(float(total), -0.2) * float(iqr) / 1.34))
    if 6 * bw + 1 > n:
        bw = max(3, (n - 1) // 6)
    reach = 3 * bw
    bell = [math.exp(-(((i - reach) / bw) ** 2) / 2) / math.sqrt(2 * math.pi) for i in range(2 * reach + 1)] + [0.0] * reach
    out = []
    for b in range(n):
        lo, k = (b - reach, 0) if b > reach else (0, b)
        s = 0.0
        for j in range(lo, min(b + reach, n)):
            s += bins[j] * bell[k]
            k += 1
        out.append(int(s / bw))
    return out


def test_smoothing_of_few_bins_reads_zeros_behind_the_weights(api):
    """with fewer bins than three cut-offs the windows of the low bins run past the last weight: zeros, not memory"""
    sizes = [298, 299, 300, 301, 302] * 8                     # 12 bins of width 1 from 294, reach 9
    h = api.InsertHistogram.from_sample(sizes)
    bins = [sizes.count(294 + b) for b in range(12)]
    assert [h.count(294 + b, smoothed=True)[0] for b in range(12)] == _smoothed_by_the_rule(bins)
    h.close()
    wide = [250 + (i * 37) % 101 for i in range(400)]         # 60 bins, reach above 9
    h = api.InsertHistogram.from_sample(wide)
    lo, hi, nb, _ = h.bounds()
    width = (hi - lo + 1) // nb
    bins = [h.count(lo + b * width, smoothed=False)[0] for b in range(nb)]
    assert nb > 16 and [h.count(lo + b * width, smoothed=True)[0] for b in range(nb)] == _smoothed_by_the_rule(bins)
    h.close()
