// smg_inshist.hpp -- the distribution of insert sizes of a read-pair library (host code; at most 1028 bins): what the
// reference keeps in insert.c, stated here over flat arrays.
//
//   SAMPLE      `smalt sample` maps every n-th pair; n follows from the number of pairs and -u (sampling_interval).
//   BINS        from a sample of insert sizes: median and quartiles of the sorted sample, six inter-quartile ranges around
//               the median cut into 3 * sqrt(sample size) bins (16 .. 1028) of a whole-numbered width (from_sample).
//   SMOOTHING   the bin counts convolved with a Gaussian whose bandwidth follows from the inter-quartile range of the
//               binned counts and their number (smooth).  The results are truncated to whole counts; the window of the
//               convolution is one bin short on its upper side and, for the lowest bins, starts at the wrong weight.  All of it
//               is part of what the pairing sees, so it is kept.
//   QUERIES     count and cumulative count of an insert size, raw or smoothed (count_of, cumulative_of).
//   TEXT        the two bar prints, the file section and its reader (print, section, parse).
// Double arithmetic through libm in the reference's order of operations: compile without fused multiply-adds.
#ifndef SMG_INSHIST_HPP
#define SMG_INSHIST_HPP
#include <stdint.h>

#include <string>
#include <vector>

namespace smginshist {

enum { TARGET_SAMPLE = 4098, BINS_MIN = 16, BINS_MAX = 1028, BINS_DEFAULT = 128, RANGE_IN_IQR = 3, BANDWIDTH_MIN = 3, BANDWIDTHS_CUT = 3, LINE_CHUNK = 126 };

// every how many pairs one is mapped (insert.c:192-205)
int sampling_interval(uint64_t npairs, int every);

struct Histogram {
  std::vector<int32_t> raw, smoothed;        // one entry per bin
  bool is_smoothed = false;
  int32_t bin_width = 1, lo = 0, hi = 0;     // insert sizes lo .. hi inclusive; bin b starts at lo + b * bin_width
  uint64_t total = 0;                        // sum of raw
  int32_t median = 0, quart_lo = 0, quart_hi = 0;

  int32_t nbins() const { return (int32_t)raw.size(); }
  // the sample is sorted in place.  false: no histogram (empty sample, or fewer than 2 sizes inside the range)
  bool from_sample(std::vector<int32_t> &sample);
  bool smooth();
  int bin_of(int32_t insert_size) const;     // for lo <= insert_size <= hi
  int32_t count_of(int32_t insert_size, bool want_smoothed) const;
  int32_t cumulative_of(int32_t insert_size, bool want_smoothed) const;
  // bars of at most `width` characters over the occupied bins; false (and the reference's one line): nothing to print
  bool print(std::string &out, int width, bool want_smoothed) const;
  bool section(std::string &out) const;      // false: the counts do not add up to `total`
  // the section of a file's text; everything ahead of its first line is skipped.  nullptr = fine, else what is wrong
  const char *parse(const char *text, size_t len);
};
void print_empty(std::string &out);

}  // namespace smginshist

// the handle of the C ABI (include/smaltgpu.h); `text` backs smaltgpu_inshist_text
struct smaltgpu_inshist {
  smginshist::Histogram h;
  std::string text;
};
#endif
