// jpeg_entropy_check -- drives csrc/jpegx_entropy.h alone (no HIP, no library) over every file of a directory; meant to be built with
// -fsanitize=address,undefined (tests/test_jpeg_cpu.py does).  Each file is probed, then decoded twice: into a heap buffer of
// EXACTLY the probed size (a write past it is the sanitizer's to report) and into a buffer with guard bytes behind the probed size
// (checked here).  A file is "taken" or "deferred", never anything else; a deferral must leave descriptor and record untouched.
// Every descriptor a file is taken with passes jpegx::desc_consistent -- the bounds check in front of the device stages -- with the
// right MCU count, and fails it once a field the kernels index with is off by one.
// Prints, per first letter of the file names, "prefix <letter> <taken>/<files>", then "jpeg entropy ok".
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "jpegx_entropy.h"

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                 \
      ++failures;                   \
    }                               \
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

// `d` as probe() / decode() wrote it: consistent, and no longer so with one field bumped
static void check_descriptor(const char* name, const char* who, const jpegx::Desc& d) {
  long long mcus = -1;
  const bool ok = jpegx::desc_consistent(d, &mcus);
  // the MCU grid from the image size alone, not from the block counts the check compares it with
  const long long want = (long long)((d.width + 8 * d.hs - 1) / (8 * d.hs)) * ((d.height + 8 * d.vs - 1) / (8 * d.vs));
  CHECK(ok && mcus == want, "%s: %s's descriptor is not consistent, or %lld MCUs for %lld", name, who, mcus, want);
  long long unused;
  jpegx::Desc b = d;
  // width + 1 is another image of the same geometry unless it opens a new MCU column: the check must tell exactly that ...
  b.width += 1;
  CHECK(jpegx::desc_consistent(b, &unused) == (d.width % (8 * d.hs) != 0), "%s: %s's width + 1 judged wrongly", name, who);
  // ... and the first width of the next MCU column never passes
  b.width = d.bw[0] * 8 + 1;
  CHECK(!jpegx::desc_consistent(b, &unused), "%s: %s's width in the next MCU column was accepted", name, who);
  b = d, b.hs += 1;
  CHECK(!jpegx::desc_consistent(b, &unused), "%s: %s's hs + 1 was accepted", name, who);
  b = d, b.bw[0] += 1;
  CHECK(!jpegx::desc_consistent(b, &unused), "%s: %s's bw[0] + 1 was accepted", name, who);
  if (d.ncomp == 3) {  // (a grayscale image has no second plane: no stage reads bh[1] of it)
    b = d, b.bh[1] += 1;
    CHECK(!jpegx::desc_consistent(b, &unused), "%s: %s's bh[1] + 1 was accepted", name, who);
  }
  b = d, b.blocks += 1;
  CHECK(!jpegx::desc_consistent(b, &unused), "%s: %s's blocks + 1 was accepted", name, who);
  b = d, b.coef_off += 1;
  CHECK(!jpegx::desc_consistent(b, &unused), "%s: %s's coef_off + 1 was accepted", name, who);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: jpeg_entropy_check DIR\n");
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
  std::map<char, std::pair<int, int>> counts;  // letter -> (taken, files)
  constexpr int MAX_SIDE = 8192;
  constexpr size_t GUARD = 64;
  for (const std::string& name : names) {
    const std::vector<uint8_t> bytes = slurp(std::string(argv[1]) + "/" + name);
    // an exact-size copy of the input too: a read past the file is the sanitizer's to report
    uint8_t* in = static_cast<uint8_t*>(malloc(bytes.size() ? bytes.size() : 1));
    std::copy(bytes.begin(), bytes.end(), in);
    jpegx::Desc probed, d;
    memset(&probed, 0x5A, sizeof(probed));
    const jpegx::Desc untouched = probed;
    const jpegx::Status p = jpegx::probe(in, bytes.size(), MAX_SIDE, &probed);
    CHECK(p == jpegx::TAKEN || p == jpegx::DEFERRED, "%s: probe status %d", name.c_str(), (int)p);
    if (p == jpegx::DEFERRED) CHECK(memcmp(&probed, &untouched, sizeof(probed)) == 0, "%s: a deferring probe wrote", name.c_str());
    const size_t size = p == jpegx::TAKEN ? jpegx::record_bytes(probed) : 4096;
    if (p == jpegx::TAKEN)
      CHECK(probed.blocks > 0 && probed.width >= 1 && probed.width <= MAX_SIDE && probed.height >= 1 && probed.height <= MAX_SIDE,
            "%s: descriptor out of range", name.c_str());
    if (p == jpegx::TAKEN) check_descriptor(name.c_str(), "probe", probed);
    // 1: exactly the probed size
    uint8_t* exact = static_cast<uint8_t*>(malloc(size));
    memset(exact, 0xA5, size);
    d = untouched;
    const jpegx::Status s1 = jpegx::decode(in, bytes.size(), MAX_SIDE, &d, exact, size);
    CHECK(s1 == jpegx::TAKEN || s1 == jpegx::DEFERRED, "%s: decode status %d", name.c_str(), (int)s1);
    CHECK(!(p == jpegx::DEFERRED && s1 == jpegx::TAKEN), "%s: decoded what the probe deferred", name.c_str());
    if (s1 == jpegx::DEFERRED) {
      bool clean = memcmp(&d, &untouched, sizeof(d)) == 0;
      for (size_t i = 0; i < size && clean; ++i) clean = exact[i] == 0xA5;
      CHECK(clean, "%s: a deferring decode wrote", name.c_str());
    } else {
      CHECK(jpegx::record_bytes(d) == size && d.blocks == probed.blocks && d.width == probed.width && d.height == probed.height,
            "%s: decode and probe disagree", name.c_str());
      check_descriptor(name.c_str(), "decode", d);
    }
    // 2: guard bytes behind the probed size; a buffer one byte short must be refused
    uint8_t* guarded = static_cast<uint8_t*>(malloc(size + GUARD));
    memset(guarded, 0xA5, size + GUARD);
    const jpegx::Status s2 = jpegx::decode(in, bytes.size(), MAX_SIDE, &d, guarded, size);
    CHECK(s2 == s1, "%s: two decodes of one file disagree", name.c_str());
    for (size_t i = 0; i < GUARD; ++i) CHECK(guarded[size + i] == 0xA5, "%s: guard byte %zu overwritten", name.c_str(), i);
    if (s1 == jpegx::TAKEN) {
      CHECK(memcmp(exact, guarded, size) == 0, "%s: two decodes of one file differ", name.c_str());
      CHECK(jpegx::decode(in, bytes.size(), MAX_SIDE, &d, guarded, size - 1) == jpegx::DEFERRED, "%s: a short buffer was accepted", name.c_str());
    }
    free(guarded);
    free(exact);
    free(in);
    auto& c = counts[name[0]];
    c.first += s1 == jpegx::TAKEN;
    c.second += 1;
  }
  for (const auto& kv : counts) printf("prefix %c %d/%d\n", kv.first, kv.second.first, kv.second.second);
  if (failures) {
    printf("%d check(s) FAILED\n", failures);
    return 1;
  }
  printf("jpeg entropy ok\n");
  return 0;
}
