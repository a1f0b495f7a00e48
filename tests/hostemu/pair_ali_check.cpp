// tests/hostemu/pair_ali_check.cpp -- TEST DRIVER (no device): pair_check.cpp's replay of the reference's recorded mapping calls
// into the product's pair logic, with the reference sequences themselves at hand, for the alignment blocks of `smalt map -a`
// (SMALTGPU_REP_ALIOUT; tests/test_report_ali.py).  The replay (ReplayExec) is pair_check.cpp's own, included here; this file adds
// the FASTA text of the reference, packed as the index holds it, and hands it to smaltgpu_report_set_reference.
//
//   pair_ali_check <refdump.txt> <reads_1.fq> <reads_2.fq> <reference.fa> key=value ...
//   keys: those of pair_check, and  ali=1 (set the flag)  noref=1 (do not hand over the reference: the emit call must fail)
#define main pair_check_main
#include "pair_check.cpp"
#undef main

// names, offsets and the packed words of a FASTA text: 10 bases per word, 3 bits each, the first base in bits 29-27, 7 behind the last
static void load_reference(const char *path, std::vector<std::string> &names, std::vector<uint64_t> &sop, std::vector<uint32_t> &packed) {
  std::ifstream f(path);
  std::string ln, all;
  sop.assign(1, 0);
  while (std::getline(f, ln)) {
    while (!ln.empty() && isspace((unsigned char)ln.back())) ln.pop_back();
    if (ln.empty()) continue;
    if (ln[0] == '>') {
      if (!names.empty()) sop.push_back(all.size());
      names.push_back(ln.substr(1, ln.find_first_of(" \t") == std::string::npos ? std::string::npos : ln.find_first_of(" \t") - 1));
    } else all += ln;
  }
  sop.push_back(all.size());
  packed.assign(all.size() / 10 + 1, 0);
  for (size_t i = 0; i <= all.size(); i++) {
    unsigned code = 7;
    if (i < all.size()) { const int c = toupper((unsigned char)all[i]); code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : (c == 'T' || c == 'U') ? 3 : 5; }
    packed[i / 10] |= code << (3 * (9 - (unsigned)(i % 10)));
  }
}

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: pair_ali_check refdump reads1 reads2 reference.fa key=value...\n"); return 2; }
  std::map<std::string, std::string> kv;
  for (int a = 5; a < argc; a++) { const char *e = strchr(argv[a], '='); if (e) kv[std::string((const char *)argv[a], (size_t)(e - argv[a]))] = e + 1; }
  auto geti = [&](const char *k, int dflt) { return kv.count(k) ? atoi(kv[k].c_str()) : dflt; };
  std::vector<RecPair> rec = load_dump(argv[1]);
  smaltgpu_reads *rs[2] = {smaltgpu_reads_create(), smaltgpu_reads_create()};
  smaltgpu_reads_view v[2];
  std::string text[2] = {slurp(argv[2]), slurp(argv[3])};
  for (int w = 0; w < 2; w++) if (smaltgpu_reads_parse(rs[w], text[w].data(), text[w].size(), 1, 0, 1, &v[w])) { fprintf(stderr, "parse: %s\n", smaltgpu_last_error()); return 1; }
  if (v[0].nreads != v[1].nreads || v[0].nreads != rec.size()) { fprintf(stderr, "pair counts differ: %u %u %zu\n", v[0].nreads, v[1].nreads, rec.size()); return 1; }
  std::vector<std::string> names;
  std::vector<uint64_t> sop;
  std::vector<uint32_t> packed;
  load_reference(argv[4], names, sop, packed);
  std::vector<const char *> name_ptr;
  for (const std::string &s : names) name_ptr.push_back(s.c_str());

  BlockInput in;
  for (int w = 0; w < 2; w++) { in.bases[w] = v[w].bases; in.quals[w] = v[w].has_qual ? v[w].quals : nullptr; in.off[w] = v[w].read_off; }
  in.npairs = v[0].nreads;
  BlockParams bp;
  memset(&bp.map, 0, sizeof(bp.map));
  bp.map.match = 1; bp.map.mismatch = -2; bp.map.gap_init = -4; bp.map.gap_ext = -3;
  bp.d_min = geti("dmin", 0); bp.d_max = geti("dmax", 500); bp.lib = geti("lib", 1); bp.every_pair = geti("every", 0) != 0; bp.k = geti("k", 13);
  bp.sop = sop.data(); bp.nseq = (int64_t)names.size(); bp.packed_host = nullptr; bp.nthreads = geti("threads", 1);
  smaltgpu_pairs *ps = smaltgpu_pairs_create();
  ReplayExec ex{rec, &in, bp.k};
  if (!ps->blk.run(ex, in, bp)) { fprintf(stderr, "pair_ali_check: %s\n", ps->blk.error.c_str()); return 1; }

  smaltgpu_report_opts ro;
  memset(&ro, 0, sizeof(ro));
  ro.format = geti("fmt", 0); ro.modflags = (uint32_t)geti("mod", 0) & ~(uint32_t)SMALTGPU_REP_HEADER; ro.outflags = (uint32_t)geti("out", 3); ro.min_swscor = geti("minsw", 18);
  ro.min_swscor_below_max = geti("below", 0); ro.min_identity = kv.count("minid") ? atof(kv["minid"].c_str()) : 0.0;
  if (geti("ali", 0)) ro.modflags |= SMALTGPU_REP_ALIOUT;
  smaltgpu_pair_opts po;
  po.insert_min = bp.d_min; po.insert_max = bp.d_max; po.library = bp.lib; po.every_pair = bp.every_pair; po.nthreads = bp.nthreads;
  if (ro.outflags & SMALTGPU_OUT_RANDSEL) srand48(geti("seed", 1));
  smaltgpu_report *rep = smaltgpu_report_create();
  const char *out; uint64_t len;
  if (smaltgpu_report_header(rep, name_ptr.data(), sop.data(), (int64_t)names.size(), &ro, "pair_ali_check", "0", 0, nullptr, &out, &len)) { fprintf(stderr, "header: %s\n", smaltgpu_last_error()); return 1; }
  if (!geti("noref", 0) && smaltgpu_report_set_reference(rep, packed.data())) { fprintf(stderr, "reference: %s\n", smaltgpu_last_error()); return 1; }
  if (smaltgpu_report_emit_pairs(rep, ps, &v[0], &v[1], name_ptr.data(), (int64_t)names.size(), &ro, &po, bp.nthreads, &out, &len)) { fprintf(stderr, "emit: %s\n", smaltgpu_last_error()); return 1; }
  fwrite(out, 1, len, stdout);
  return 0;
}
