// tests/hostemu/alnin_check.cpp -- TEST DRIVER (no device, no library): smalt_amd/csrc/smg_alnin.hpp on its own, meant to be built with
// -fsanitize=address,undefined and run directly (tests/test_alnin.py).
//
//   alnin_check <jobs.txt> <small.bam>
//
// Every line of <jobs.txt> is "<sam|bam> <file> <threads> <window> <max_templates>": the file is fed to a reader in windows of <window>
// bytes (0: whole; a window grows by its size until the reader uses some of it), the runs are taken after every feed, and the line
// "job ok <templates> <crc32>" is printed -- the checksum runs over every template: its kind, whether its run has qualities, and name,
// bases and qualities of its reads -- or "job error <message>" when the reader refuses the file.  The windows are copied into
// buffers of exactly their size, so that a read past a window is a read past an allocation.
// Then every prefix of <small.bam> is decoded as if it were the whole file: "prefixes: <n> cut, <clean> clean, <errors> errors".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>

#include "../../smalt_amd/csrc/smg_alnin.hpp"

static std::string slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

static void put32(unsigned char *o, uint32_t v) { for (int k = 0; k < 4; k++) o[k] = (unsigned char)(v >> (8 * k)); }

// -> true: decoded to the end; false: the reader refused (why)
static bool run(int format, const std::string &data, int nthreads, size_t window, uint32_t max_templates, uint64_t *ntemplates, uint32_t *crc, std::string *why) {
  smgaln::Reader rd;
  rd.format = format;
  const size_t step = window ? window : (data.size() ? data.size() : 1);
  size_t pos = 0, cur = step;
  uLong c = crc32(0L, Z_NULL, 0);
  *ntemplates = 0;
  for (;;) {
    const bool last = pos + cur >= data.size();
    const size_t n = last ? data.size() - pos : cur;
    char *win = (char *)malloc(n ? n : 1);                    // exactly the window
    if (n) memcpy(win, data.data() + pos, n);
    uint64_t used = 0;
    const int rv = rd.feed(win, n, last, nthreads, &used);
    free(win);
    if (rv) { *why = rd.err; return false; }
    if (used > n || (last && used != n)) { *why = "(driver) consumed more than the window, or not all of the last one"; return false; }
    pos += used;
    for (;;) {
      int kind = 0;
      const uint32_t nt = rd.take(max_templates, &kind);
      if (!kind) break;
      for (uint32_t i = 0; i < nt; i++) {
        unsigned char head[8];
        put32(head, (uint32_t)kind); put32(head + 4, rd.run_has_qual ? 1u : 0u);
        c = crc32(c, head, 8);
        for (int s = 0; s < kind; s++) {
          const smgaln::Side &sd = rd.side[s];
          c = crc32(c, (const Bytef *)sd.names.data() + sd.name_off[i], (uInt)(sd.name_off[i + 1] - sd.name_off[i]));
          c = crc32(c, sd.bases.data() + sd.off[i], (uInt)(sd.off[i + 1] - sd.off[i]));
          if (rd.run_has_qual) c = crc32(c, sd.quals.data() + sd.off[i], (uInt)(sd.off[i + 1] - sd.off[i]));
        }
      }
      *ntemplates += nt;
    }
    if (last) break;
    cur = used ? step : cur + step;
  }
  *crc = (uint32_t)c;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: alnin_check <jobs.txt> <small.bam>\n"); return 2; }
  std::ifstream jobs(argv[1]);
  std::string fmt, path;
  long nthreads, window, max_templates;
  while (jobs >> fmt >> path >> nthreads >> window >> max_templates) {
    const std::string data = slurp(path);
    uint64_t n; uint32_t crc; std::string why;
    if (run(fmt == "sam" ? smgaln::FMT_SAM : smgaln::FMT_BAM, data, (int)nthreads, (size_t)window, (uint32_t)max_templates, &n, &crc, &why))
      printf("job ok %llu %08x\n", (unsigned long long)n, crc);
    else printf("job error %s\n", why.c_str());
  }
  const std::string small = slurp(argv[2]);
  size_t clean = 0, errors = 0;
  for (size_t cut = 0; cut < small.size(); cut++) {
    uint64_t n; uint32_t crc; std::string why;
    if (run(smgaln::FMT_BAM, small.substr(0, cut), 1 + (int)(cut % 3), cut % 5 == 0 ? 0 : 1 + cut % 97, 0, &n, &crc, &why)) clean++; else errors++;
  }
  printf("prefixes: %zu cut, %zu clean, %zu errors\n", small.size(), clean, errors);
  return 0;
}
