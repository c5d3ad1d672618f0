// jpeg_split_check -- drives csrc/jpegx_split.h (the self-synchronising decode inside a restart interval) against the
// serial interval decoder of csrc/jpegx_scan.h over every file of a directory, with no HIP and no library; meant to be built with
// -fsanitize=address,undefined (tests/test_jpeg_split_cpu.py does).  For each file the scan preparation takes, and each
// split_bytes in {32, 128, 1024} with max_rounds in {1, 4096}:
//   1. every interval is decoded serially (the device sink's rules: range judged at a block's end) into a buffer of exactly the
//      record's size, and by the rule of the cut into a second one pre-filled with a pattern;
//   2. the two codes are equal, interval for interval;
//   3. when all are clean the two buffers are equal byte for byte, and equal to jpegx::decode's record when it takes the file;
//   4. rounds: 0 exactly when the interval is shorter than 2 x split_bytes, -1 at max_rounds 1, and 2 .. sub-sequences + 1 at 4096.
// Prints, per first letter of the file names, "prefix <letter> <files> <prepared> <split intervals> <most rounds>", then
// "jpeg split ok".
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "jpegx_entropy.h"
#include "jpegx_scan.h"
#include "jpegx_split.h"

namespace S = jpegx::scan;
namespace P = jpegx::scan::split;

static int failures = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                   \
      ++failures;                     \
    }                                 \
  } while (0)

static std::vector<uint8_t> slurp(const std::string& path) {
  std::vector<uint8_t> out;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return out;
  uint8_t buf[1 << 14];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return out;
}

struct Count {
  int files = 0, prepared = 0, split = 0, most = 0;
};

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: jpeg_split_check DIR\n");
    return 2;
  }
  std::vector<std::string> names;
  DIR* dir = opendir(argv[1]);
  if (!dir) {
    perror(argv[1]);
    return 2;
  }
  while (dirent* e = readdir(dir))
    if (e->d_name[0] != '.') names.push_back(e->d_name);
  closedir(dir);
  std::sort(names.begin(), names.end());
  std::map<char, Count> counts;
  constexpr int MAX_SIDE = 8192;
  const uint32_t splits[3] = {32, 128, 1024};
  const int caps[2] = {1, 4096};
  for (const std::string& name : names) {
    const char* nm = name.c_str();
    const std::vector<uint8_t> bytes = slurp(std::string(argv[1]) + "/" + name);
    Count& cnt = counts[name[0]];
    cnt.files += 1;
    jpegx::Desc d;
    size_t size = 0;
    if (S::probe(bytes.data(), bytes.size(), MAX_SIDE, &d, &size) != jpegx::TAKEN) continue;
    uint8_t* rec = static_cast<uint8_t*>(malloc(size));  // exact size: a read past the record is reported
    if (S::prepare(bytes.data(), bytes.size(), MAX_SIDE, &d, rec, size) != jpegx::TAKEN) {
      free(rec);
      continue;
    }
    cnt.prepared += 1;
    S::ScanHeader h;
    memcpy(&h, rec, sizeof(h));
    CHECK(S::header_fits(h, S::intervals_of(d), size), "%s: the record's header does not describe it", nm);
    const S::Geometry g = P::geometry_of(d, h);
    const S::HuffDev* tab = reinterpret_cast<const S::HuffDev*>(rec + S::TAB_OFF);
    const S::Interval* ivl = reinterpret_cast<const S::Interval*>(rec + S::ivl_off(h.ntables));
    const uint8_t* file = rec + S::file_off(h.ntables, h.nintervals);
    const size_t ncoef = (size_t)d.blocks * 64;

    // the references: the serial decoder, interval by interval, and the host entropy stage
    int16_t* serial = static_cast<int16_t*>(calloc(ncoef, sizeof(int16_t)));
    P::MemPlanes ms;
    ms.set(reinterpret_cast<const uint16_t*>(rec + S::QT_OFF), serial, d);
    std::vector<int> want((size_t)h.nintervals);
    bool all_clean = true;
    for (int i = 0; i < h.nintervals; ++i) {
      P::RowSink sink;
      sink.m = ms;
      want[i] = S::decode_interval(P::MemSrc{file}, g, tab, ivl[i].begin, ivl[i].end, ivl[i].first_mcu, ivl[i].nmcu, sink);
      all_clean = all_clean && want[i] == S::CLEAN;
    }
    jpegx::Desc rd;
    std::vector<uint8_t> ref(jpegx::record_bytes(d));
    const bool host_takes = jpegx::decode(bytes.data(), bytes.size(), MAX_SIDE, &rd, ref.data(), ref.size()) == jpegx::TAKEN;
    CHECK(host_takes == all_clean, "%s: host stage %d, serial intervals %d", nm, (int)host_takes, (int)all_clean);
    if (host_takes) CHECK(memcmp(ref.data() + jpegx::TABLE_BYTES, serial, ncoef * 2) == 0, "%s: the serial record differs from the host stage's", nm);

    for (const uint32_t sb : splits)
      for (const int cap : caps) {
        int16_t* coef = static_cast<int16_t*>(malloc(ncoef * sizeof(int16_t)));  // exact size
        memset(coef, 0xA5, ncoef * sizeof(int16_t));
        P::MemPlanes m;
        m.set(reinterpret_cast<const uint16_t*>(rec + S::QT_OFF), coef, d);
        for (int i = h.nintervals - 1; i >= 0; --i) {
          const uint32_t E = ivl[i].end - ivl[i].begin;
          int rounds = 12345;
          const int code = P::decode_interval_host(file, g, tab, ivl[i], m, sb, cap, &rounds);
          CHECK(code == want[i], "%s: split %u cap %d interval %d: code %d, serial %d", nm, sb, cap, i, code, want[i]);
          const P::Cut cut = P::cut_of(E, sb);
          CHECK((cut.nsub != 0) == (E >= 2 * sb), "%s: split %u interval %d of %u bytes: %d sub-sequences", nm, sb, i, E, cut.nsub);
          if (cut.nsub == 0)
            CHECK(rounds == 0, "%s: split %u interval %d: rounds %d of an interval that is not split", nm, sb, i, rounds);
          else if (cap == 1)
            CHECK(rounds == -1, "%s: split %u cap 1 interval %d: rounds %d", nm, sb, i, rounds);
          else
            CHECK(rounds >= 2 && rounds <= cut.nsub + 1, "%s: split %u interval %d: rounds %d, %d sub-sequences", nm, sb, i, rounds, cut.nsub);
          if (cut.nsub && cap != 1 && sb == 32) {
            cnt.split += 1;
            cnt.most = std::max(cnt.most, rounds);
          }
        }
        if (all_clean) CHECK(memcmp(coef, serial, ncoef * 2) == 0, "%s: split %u cap %d: the record differs from the serial decoder's", nm, sb, cap);
        free(coef);
      }
    free(serial);
    free(rec);
  }
  for (const auto& kv : counts) printf("prefix %c %d %d %d %d\n", kv.first, kv.second.files, kv.second.prepared, kv.second.split, kv.second.most);
  if (failures) {
    printf("%d check(s) FAILED\n", failures);
    return 1;
  }
  printf("jpeg split ok\n");
  return 0;
}
