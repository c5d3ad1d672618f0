// jpeg_scan_check -- drives csrc/jpegx_scan.h (host preparation + the interval decoder the GPU kernel instantiates) against
// csrc/jpegx_entropy.h over every file of a directory, with no HIP and no library; meant to be built with
// -fsanitize=address,undefined (tests/test_jpeg_huffman_cpu.py does).  For each file:
//   1. the scan record is prepared into a heap buffer of EXACTLY the probed size (a write past it is the sanitizer's to report) and
//      into a buffer with guard bytes behind that size (checked here); a deferral must leave descriptor and record untouched;
//   2. every interval is decoded with the shared decoder from the exact-size record (a read past it is the sanitizer's), in
//      REVERSE order, into a coefficient buffer of exactly the record's size;
//   3. jpegx::decode TAKEN  <=>  preparation TAKEN and every interval clean;
//   4. when taken, [tables | coefficients] equals jpegx::decode's record byte for byte.
// Prints, per first letter of the file names, "prefix <letter> <taken>/<files> <reached the interval decoder> <of those, not clean>",
// then "jpeg scan ok".
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "jpegx_entropy.h"
#include "jpegx_scan.h"

namespace S = jpegx::scan;

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

struct MemSrc {  // the file bytes of a record
  const uint8_t* base;
  unsigned byte(uint32_t pos) const { return base[pos]; }
};

struct MemSink {  // the host stage's stores: range guard at once, natural order
  const uint16_t* qt;
  int16_t* plane[3];
  const uint16_t* q;
  int16_t* out;
  void begin(int c, long long blk) {
    q = qt + 64 * c;
    out = plane[c] + blk * 64;
  }
  bool put(int k, int v) {
    const int nat = jpegx::detail::NATURAL[k];
    if (v * (int)q[nat] > jpegx::MAX_ABS_DEQUANT || v * (int)q[nat] < -jpegx::MAX_ABS_DEQUANT) return false;
    out[nat] = (int16_t)v;
    return true;
  }
  bool end() { return true; }
};

struct Count {
  int taken = 0, files = 0, reached = 0, unclean = 0;
};

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: jpeg_scan_check DIR\n");
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
  constexpr size_t GUARD = 64;
  for (const std::string& name : names) {
    const char* nm = name.c_str();
    const std::vector<uint8_t> bytes = slurp(std::string(argv[1]) + "/" + name);
    uint8_t* in = static_cast<uint8_t*>(malloc(bytes.size() ? bytes.size() : 1));  // exact size: a read past the file is reported
    std::copy(bytes.begin(), bytes.end(), in);

    // the reference: the host entropy stage
    jpegx::Desc rd;
    std::vector<uint8_t> ref;
    jpegx::Status s_ref = jpegx::probe(in, bytes.size(), MAX_SIDE, &rd);
    if (s_ref == jpegx::TAKEN) {
      ref.resize(jpegx::record_bytes(rd));
      s_ref = jpegx::decode(in, bytes.size(), MAX_SIDE, &rd, ref.data(), ref.size());
    }

    // 1: preparation
    jpegx::Desc probed, d;
    memset(&probed, 0x5A, sizeof(probed));
    const jpegx::Desc untouched = probed;
    size_t size = 12345;
    const jpegx::Status p = S::probe(in, bytes.size(), MAX_SIDE, &probed, &size);
    CHECK(p == jpegx::TAKEN || p == jpegx::DEFERRED, "%s: probe status %d", nm, (int)p);
    if (p == jpegx::DEFERRED) {
      CHECK(memcmp(&probed, &untouched, sizeof(probed)) == 0 && size == 12345, "%s: a deferring probe wrote", nm);
      size = 4096;
    }
    uint8_t* rec = static_cast<uint8_t*>(malloc(size));
    memset(rec, 0xA5, size);
    d = untouched;
    const jpegx::Status s1 = S::prepare(in, bytes.size(), MAX_SIDE, &d, rec, size);
    CHECK(s1 == jpegx::TAKEN || s1 == jpegx::DEFERRED, "%s: prepare status %d", nm, (int)s1);
    CHECK(!(p == jpegx::DEFERRED && s1 == jpegx::TAKEN), "%s: prepared what the probe deferred", nm);
    if (s1 == jpegx::DEFERRED) {
      bool clean = memcmp(&d, &untouched, sizeof(d)) == 0;
      for (size_t i = 0; i < size && clean; ++i) clean = rec[i] == 0xA5;
      CHECK(clean, "%s: a deferring preparation wrote", nm);
    }
    uint8_t* guarded = static_cast<uint8_t*>(malloc(size + GUARD));
    memset(guarded, 0xA5, size + GUARD);
    jpegx::Desc d2 = untouched;
    const jpegx::Status s2 = S::prepare(in, bytes.size(), MAX_SIDE, &d2, guarded, size);
    CHECK(s2 == s1, "%s: two preparations of one file disagree", nm);
    for (size_t i = 0; i < GUARD; ++i) CHECK(guarded[size + i] == 0xA5, "%s: guard byte %zu overwritten", nm, i);
    if (s1 == jpegx::TAKEN) {
      CHECK(memcmp(rec, guarded, size) == 0 && memcmp(&d, &d2, sizeof(d)) == 0, "%s: two preparations of one file differ", nm);
      CHECK(S::prepare(in, bytes.size(), MAX_SIDE, &d2, guarded, size - 1) == jpegx::DEFERRED, "%s: a short buffer was accepted", nm);
    }
    free(guarded);

    // 2: every interval on its own, last one first
    bool all_clean = false;
    if (s1 == jpegx::TAKEN) {
      S::ScanHeader h;
      memcpy(&h, rec, sizeof(h));
      const bool fits = S::header_fits(h, S::intervals_of(d), size) && h.total_bytes == size && h.file_bytes == bytes.size();
      CHECK(fits, "%s: the record's header does not describe it", nm);
      if (fits) {
        const S::HuffDev* tab = reinterpret_cast<const S::HuffDev*>(rec + S::TAB_OFF);
        const S::Interval* ivl = reinterpret_cast<const S::Interval*>(rec + S::ivl_off(h.ntables));
        const uint8_t* file = rec + S::file_off(h.ntables, h.nintervals);
        CHECK(memcmp(file, in, bytes.size()) == 0, "%s: the record does not hold the file", nm);
        S::Geometry g;
        g.ncomp = d.ncomp;
        g.hs = d.hs;
        g.vs = d.vs;
        g.mx = d.bw[0] / d.hs;
        for (int c = 0; c < 3; ++c) {
          g.bw[c] = d.bw[c];
          g.dc[c] = h.dc_tab[c];
          g.ac[c] = h.ac_tab[c];
        }
        const size_t ncoef = (size_t)d.blocks * 64;
        int16_t* coef = static_cast<int16_t*>(calloc(ncoef, sizeof(int16_t)));  // exact size
        MemSink sink;
        sink.qt = reinterpret_cast<const uint16_t*>(rec + S::QT_OFF);
        sink.plane[0] = coef;
        sink.plane[1] = sink.plane[2] = nullptr;
        for (int c = 1; c < d.ncomp; ++c) sink.plane[c] = sink.plane[c - 1] + (size_t)d.bw[c - 1] * d.bh[c - 1] * 64;
        const long long mcus = S::mcus_of(d), per = d.restart > 0 ? d.restart : mcus;
        all_clean = true;
        for (int i = h.nintervals - 1; i >= 0; --i) {
          const S::Interval& I = ivl[i];
          const bool ok = I.first_mcu == i * per && I.nmcu == std::min(per, mcus - i * per) && I.begin <= I.end && I.end <= h.file_bytes;
          CHECK(ok, "%s: interval %d of the table is off", nm, i);
          if (!ok) {
            all_clean = false;
            continue;
          }
          const int code = S::decode_interval(MemSrc{file}, g, tab, I.begin, I.end, I.first_mcu, I.nmcu, sink);
          CHECK(code >= S::CLEAN && code <= S::TRAILING && code != S::BAD_RECORD, "%s: interval %d: code %d", nm, i, code);
          all_clean = all_clean && code == S::CLEAN;
        }
        // 3 + 4
        if (all_clean && s_ref == jpegx::TAKEN) {
          CHECK(memcmp(&d, &rd, sizeof(d)) == 0, "%s: the descriptors differ", nm);
          CHECK(ref.size() == jpegx::TABLE_BYTES + ncoef * 2 && memcmp(ref.data(), rec + S::QT_OFF, jpegx::TABLE_BYTES) == 0 &&
                    memcmp(ref.data() + jpegx::TABLE_BYTES, coef, ncoef * 2) == 0,
                "%s: the record differs from the host stage's", nm);
        }
        free(coef);
      }
    }
    CHECK((s_ref == jpegx::TAKEN) == (s1 == jpegx::TAKEN && all_clean), "%s: host stage %s, scan %s / intervals %s", nm,
          s_ref == jpegx::TAKEN ? "TAKEN" : "DEFERRED", s1 == jpegx::TAKEN ? "TAKEN" : "DEFERRED", all_clean ? "clean" : "not clean");
    free(rec);
    free(in);
    Count& c = counts[name[0]];
    c.taken += s_ref == jpegx::TAKEN;
    c.files += 1;
    c.reached += s1 == jpegx::TAKEN;
    c.unclean += s1 == jpegx::TAKEN && !all_clean;
  }
  for (const auto& kv : counts) printf("prefix %c %d/%d %d %d\n", kv.first, kv.second.taken, kv.second.files, kv.second.reached, kv.second.unclean);
  if (failures) {
    printf("%d check(s) FAILED\n", failures);
    return 1;
  }
  printf("jpeg scan ok\n");
  return 0;
}
