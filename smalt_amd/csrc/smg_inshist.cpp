// smg_inshist.cpp -- insert-size histograms (smg_inshist.hpp) and their entry points of the C ABI (include/smaltgpu.h).
#include "smg_inshist.hpp"

#include <ctype.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/smaltgpu.h"

extern "C" int smaltgpu_set_error(int code, const char *msg);   // smaltgpu.cpp

namespace smginshist {

int sampling_interval(uint64_t npairs, int every) {
  const uint64_t n = npairs / TARGET_SAMPLE;
  int interval = n < 1 ? 1 : (n > (uint64_t)INT_MAX ? INT_MAX : (int)n);
  if (every > 0 && every < interval) interval = every;
  return interval;
}

bool Histogram::from_sample(std::vector<int32_t> &sample) {
  *this = Histogram();
  const size_t ns = sample.size();
  if (!ns || ns > (size_t)INT_MAX) return false;
  std::sort(sample.begin(), sample.end());
  median = sample[(size_t)((double)ns * .5)];
  quart_lo = sample[(size_t)((double)ns * .25)];
  quart_hi = sample[(size_t)((double)ns * .75)];
  int32_t range = (quart_hi - quart_lo) * RANGE_IN_IQR * 2;
  int32_t bins = (int32_t)(3 * sqrt((double)(int32_t)ns));
  bins = bins < BINS_MIN ? BINS_MIN : (bins > BINS_MAX ? BINS_MAX : bins);
  bin_width = range / bins;
  if (bin_width < 1) { bins = range; bin_width = 1; }
  else range = bin_width * bins;
  raw.assign((size_t)(bins < 1 ? BINS_DEFAULT : bins), 0);
  smoothed.assign(raw.size(), 0);
  lo = median - range / 2;
  hi = lo + range - 1;
  for (int32_t v : sample)
    if (v >= lo && v <= hi) { raw[(size_t)bin_of(v)]++; total++; }
  return smooth();
}

int Histogram::bin_of(int32_t insert_size) const {
  const int b = (insert_size - lo) / bin_width;
  return b >= nbins() ? nbins() - 1 : b;
}

bool Histogram::smooth() {
  if (total < 2) return false;
  const int32_t n = nbins();
  // inter-quartile range of the binned counts, in bins: each quartile found gives half of its bin's count back
  int32_t iqr = 0;
  if (n > 3) {
    int32_t run = 0, mark = (int32_t)(total / 4), at[3] = {0, 0, 0};
    int found = 0;
    for (int32_t b = 0; b < n && found < 3; b++) {
      run += raw[(size_t)b];
      if (run > mark) {
        at[found++] = b;
        run -= raw[(size_t)b] / 2;
        mark = (int32_t)(total * (uint64_t)found / 4);
      }
    }
    if (found > 2) iqr = at[2] - at[0];
  }
  const int32_t count = (int32_t)total;
  int32_t bw = count > 0 ? (int32_t)(0.9 * pow((double)count, -0.2) * ((double)iqr) / 1.34) : 0;
  if (bw < BANDWIDTH_MIN) bw = BANDWIDTH_MIN;
  if (2 * BANDWIDTHS_CUT * bw + 1 > n) bw = (n - 1) / (2 * BANDWIDTHS_CUT);
  if (bw < BANDWIDTH_MIN) bw = BANDWIDTH_MIN;
  const int32_t reach = BANDWIDTHS_CUT * bw;
  // the weights are indexed from the bin's own number for the bins below `reach` (not from reach - b), which runs up to weight
  // 3 * reach - 2: the reference finds zeros of its zero-filled buffer there, so there are zeros here
  std::vector<double> bell((size_t)(3 * reach + 1), 0.0);
  const double norm = sqrt(2 * M_PI);
  for (int32_t i = 0; i <= 2 * reach; i++) {
    const double x = ((double)(i - reach)) / bw;
    bell[(size_t)i] = exp(-x * x / 2) / norm;
  }
  smoothed.assign((size_t)n, 0);
  for (int32_t b = 0; b < n; b++) {
    int32_t from = b > reach ? b - reach : 0, k = b > reach ? 0 : b;
    const int32_t to = b + reach < n ? b + reach : n;       // exclusive: the window stops one bin short above b
    double sum = 0.0;
    for (; from < to; from++, k++) sum += raw[(size_t)from] * bell[(size_t)k];
    smoothed[(size_t)b] = (int32_t)(sum / bw);
  }
  is_smoothed = true;
  return true;
}

int32_t Histogram::count_of(int32_t insert_size, bool want_smoothed) const {
  if (insert_size < lo || insert_size > hi || raw.empty()) return 0;
  return (want_smoothed && is_smoothed ? smoothed : raw)[(size_t)bin_of(insert_size)];
}

int32_t Histogram::cumulative_of(int32_t insert_size, bool want_smoothed) const {
  if (insert_size < lo || insert_size > hi || raw.empty()) return 0;
  const std::vector<int32_t> &c = want_smoothed && is_smoothed ? smoothed : raw;
  int32_t sum = 0;
  for (int b = bin_of(insert_size); b >= 0; b--) sum += c[(size_t)b];
  return sum;
}

void print_empty(std::string &out) { out += "# Histogram of insert sizes is empty.\n"; }

bool Histogram::print(std::string &out, int width, bool want_smoothed) const {
  // the occupied stretch and the tallest bar are those of the raw counts, also for the smoothed print
  int32_t first = 0, last = 0, tallest = 0;
  const int32_t n = nbins();
  while (first < n && raw[(size_t)first] == 0) first++;
  if (first >= n) { print_empty(out); return false; }
  for (int32_t b = first; b < n; b++)
    if (raw[(size_t)b] > 0) { last = b; if (raw[(size_t)b] > tallest) tallest = raw[(size_t)b]; }
  const std::vector<int32_t> &c = want_smoothed && is_smoothed ? smoothed : raw;
  double per_count = ((double)width) / tallest;
  if (per_count > 1.0) per_count = 1.0;
  char label[32];
  for (int32_t b = first; b <= last; b++) {
    const int32_t bar = (int32_t)(c[(size_t)b] * per_count);
    snprintf(label, sizeof(label), "#%5i ", (int)(lo + b * bin_width));
    out += label;
    if (bar > 0) out.append((size_t)bar, '*');
    out.push_back('\n');
  }
  return true;
}

namespace {
const char SECTION_TITLE[] = "# SMALT histogram of insert sizes\n";
const char KEY_START[] = "HISTO_START", KEY_END[] = "HISTO_END";
const char *const KEYS[6] = {"HISTO_BINNUM", "HISTO_SCALFAC", "HISTO_INSIZLO", "HISTO_INSIZHI", "HISTO_TOTNUM", "HISTO_QUARTILES"};

// a cursor over the text that reads the way the C library's line and number readers do
struct Cursor {
  const char *p, *end;
  void skip_space() { while (p < end && isspace((unsigned char)*p)) p++; }
  bool word(const char *w) { const size_t l = strlen(w); if ((size_t)(end - p) < l || memcmp(p, w, l)) return false; p += l; return true; }
  bool integer(long long *v, int base) {      // optional white space, sign, digits (base 0: 0x.. and 0.. as well)
    skip_space();
    std::string tok;
    const char *q = p;
    if (q < end && (*q == '+' || *q == '-')) tok.push_back(*q++);
    while (q < end && isalnum((unsigned char)*q) && tok.size() < 40) tok.push_back(*q++);
    char *stop = nullptr;
    const long long x = base ? (long long)strtoull(tok.c_str(), &stop, base) : strtoll(tok.c_str(), &stop, 0);
    if (stop == tok.c_str() || (stop == tok.c_str() + 1 && !isdigit((unsigned char)tok[0]))) return false;
    p += stop - tok.c_str();
    *v = x;
    return true;
  }
  // the next stretch of at most LINE_CHUNK characters, up to and including a line end
  bool line(const char **at, size_t *len) {
    if (p >= end) return false;
    const char *q = p;
    while (q < end && (size_t)(q - p) < LINE_CHUNK) if (*q++ == '\n') break;
    *at = p; *len = (size_t)(q - p); p = q;
    return true;
  }
};
}  // namespace

bool Histogram::section(std::string &out) const {
  uint64_t sum = 0;
  for (int32_t c : raw) sum += (uint64_t)(int64_t)c;
  if (sum != total) return false;
  char buf[256];
  out += SECTION_TITLE;
  out += KEY_START; out.push_back('\n');
  snprintf(buf, sizeof(buf), "%s %i\n%s %i\n%s %i\n%s %i\n%s %llu\n%s %i %i %i\n", KEYS[0], (int)nbins(), KEYS[1], (int)bin_width, KEYS[2], (int)lo, KEYS[3], (int)hi,
           KEYS[4], (unsigned long long)sum, KEYS[5], (int)quart_lo, (int)median, (int)quart_hi);
  out += buf;
  for (int32_t b = 0; b < nbins(); b++) { snprintf(buf, sizeof(buf), "%i %i\n", (int)(lo + b * bin_width), (int)raw[(size_t)b]); out += buf; }
  out += KEY_END; out.push_back('\n');
  return true;
}

const char *Histogram::parse(const char *text, size_t len) {
  *this = Histogram();
  Cursor c{text, text + len};
  const char *at; size_t n;
  bool started = false;
  while (c.line(&at, &n)) if (n >= strlen(KEY_START) && !memcmp(at, KEY_START, strlen(KEY_START))) { started = true; break; }
  if (!started) return "no HISTO_START line";
  long long v[8];
  int got = 0;
  for (int k = 0; k < 6; k++) {
    if (k) c.skip_space();
    if (!c.word(KEYS[k])) return "the keys behind HISTO_START are not the expected ones";
    for (int j = 0; j < (k == 5 ? 3 : 1); j++) if (!c.integer(&v[got++], k == 4 ? 10 : 0)) return "a key behind HISTO_START has no number";
  }
  c.skip_space();
  const long long bins = v[0] < 1 ? BINS_DEFAULT : v[0];
  if (bins > (1 << 24)) return "HISTO_BINNUM is out of range";
  if ((int)v[1] == 0) return "HISTO_SCALFAC is 0";
  raw.assign((size_t)bins, 0);
  smoothed.assign((size_t)bins, 0);
  bin_width = (int32_t)v[1]; lo = (int32_t)v[2]; hi = (int32_t)v[3];
  const uint64_t claimed = (uint64_t)v[4];
  quart_lo = (int32_t)v[5]; median = (int32_t)v[6]; quart_hi = (int32_t)v[7];
  int32_t nread = 0;
  bool ended = false;
  const char *why = "no HISTO_END line";
  while (c.line(&at, &n)) {
    if (n >= strlen(KEY_END) && !memcmp(at, KEY_END, strlen(KEY_END))) { ended = true; break; }
    Cursor l{at, at + n};
    long long size, count;
    if (!l.integer(&size, 0) || !l.integer(&count, 0)) { why = "a bin line does not hold two numbers"; break; }
    if ((int32_t)size != lo + nread * bin_width) { why = "a bin is out of sequence"; break; }
    if (nread >= (int32_t)v[0]) { why = "more bins than HISTO_BINNUM"; break; }
    raw[(size_t)nread++] = (int32_t)count;
    total += (uint64_t)(int64_t)(int32_t)count;
  }
  if (!ended) return why;
  if (total != claimed) return "the bin counts do not add up to HISTO_TOTNUM";
  if (!smooth()) return "fewer than 2 insert sizes";
  return nullptr;
}

}  // namespace smginshist

// ---- C ABI ------------------------------------------------------------------------------------------------------------
extern "C" int smaltgpu_sample_interval(uint64_t npairs, int every) { return smginshist::sampling_interval(npairs, every); }

extern "C" int smaltgpu_inshist_from_sample(smaltgpu_inshist **out, const int32_t *sample, uint64_t n) {
  if (!out || (n && !sample)) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_inshist_from_sample: null argument");
  *out = nullptr;
  std::vector<int32_t> s(sample, sample + n);
  smaltgpu_inshist *h = new smaltgpu_inshist();
  if (!h->h.from_sample(s)) { delete h; return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_inshist_from_sample: the sample gives no histogram (fewer than 2 insert sizes inside six inter-quartile ranges)"); }
  *out = h;
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_inshist_read(smaltgpu_inshist **out, const char *path) {
  if (!out || !path) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_inshist_read: null argument");
  *out = nullptr;
  FILE *f = fopen(path, "rb");
  if (!f) { std::string m = std::string("cannot open the histogram file ") + path; return smaltgpu_set_error(SMALTGPU_EFILE, m.c_str()); }
  std::string text;
  char buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
  fclose(f);
  smaltgpu_inshist *h = new smaltgpu_inshist();
  if (const char *why = h->h.parse(text.data(), text.size())) {
    delete h;
    std::string m = std::string("histogram file ") + path + ": " + why;
    return smaltgpu_set_error(SMALTGPU_EFILE, m.c_str());
  }
  *out = h;
  return SMALTGPU_OK;
}

extern "C" void smaltgpu_inshist_free(smaltgpu_inshist *h) { delete h; }

extern "C" int smaltgpu_inshist_text(smaltgpu_inshist *h, int what, int width, const char **text, uint64_t *len) {
  if (!h || !text || !len) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_inshist_text: null argument");
  h->text.clear();
  if (what == SMALTGPU_HIST_SAMPLED || what == SMALTGPU_HIST_SMOOTHED) {
    if (width < 1) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_inshist_text: line width below 1");
    (void)h->h.print(h->text, width, what == SMALTGPU_HIST_SMOOTHED);
  } else if (what == SMALTGPU_HIST_SECTION) {
    if (!h->h.section(h->text)) return smaltgpu_set_error(SMALTGPU_EINTERNAL, "smaltgpu_inshist_text: the bin counts do not add up");
  } else return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_inshist_text: unknown kind of text");
  *text = h->text.data(); *len = h->text.size();
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_inshist_bounds(const smaltgpu_inshist *h, int32_t *lo, int32_t *hi, int32_t *nbins, uint64_t *total) {
  if (!h) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_inshist_bounds: null argument");
  if (lo) *lo = h->h.lo;
  if (hi) *hi = h->h.hi;
  if (nbins) *nbins = h->h.nbins();
  if (total) *total = h->h.total;
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_inshist_count(const smaltgpu_inshist *h, int32_t insert_size, int smoothed, int32_t *count, int32_t *cumulative) {
  if (!h) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_inshist_count: null argument");
  if (count) *count = h->h.count_of(insert_size, smoothed != 0);
  if (cumulative) *cumulative = h->h.cumulative_of(insert_size, smoothed != 0);
  return SMALTGPU_OK;
}
