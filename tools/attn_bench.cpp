// attn_bench.cpp -- times the library's attention kernel (clipx_attention_dh_device, include/clipx.h) without Python and
// checks a few (batch, head) pairs against an fp32 CPU softmax(QK^T/sqrt(dh))V of the same IEEE fp16 inputs (round 4: q, k, v are fp16; the output is bf16).
//   hipcc -O2 -o tools/attn_bench tools/attn_bench.cpp -ldl ;  tools/attn_bench [B T H dh causal [ab_cfg]]
// ab_cfg (tools library, CLIPX_LIB=libclipx_ablate.so): alternates the default dispatch and CLIPX_ATTN_CFG=ab_cfg in one process on the
// same buffers -- rounds of 20 timed launches each, A B A B ... -- and prints the median and the spread of the round medians of both,
// and the largest difference of their outputs.  ab_cfg = 19 at T = 577 .. 608: the long-sequence kernel against the RECOMP yardstick.
//   tools/attn_bench B T H 80,88,104   -- a comma list of head dimensions (not causal): the kernels of the list alternate in one
// process, rounds of 20 timed launches each (80 88 104 80 88 104 ...), buffers of their own; per head dimension the median of the
// round medians, the spread, TFLOP/s counted on the real dh, the k-steps + PV steps the kernel issues per key block
// (ceil(dh / 16) + 2 DV / 32) and the time relative to the first of the list per such step.  One (batch, head) pair of each is
// checked against the fp32 CPU softmax first.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
typedef int (*attn_fn)(int, const void*, void*, int, int, int, int, int, void*);
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
static float bf2f(uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
static float h2f(uint16_t b) { _Float16 h; memcpy(&h, &b, 2); return (float)h; }
static uint16_t f2h(float f) { _Float16 h = (_Float16)f; uint16_t b; memcpy(&b, &h, 2); return b; }
// max |out - fp32 CPU| over the (batch, head) pairs given
static double cpu_check(const std::vector<uint16_t>& hq, const std::vector<uint16_t>& ho, int T, int H, int dh, int causal, const int (*pairs)[2], int npairs) {
  const size_t ld = (size_t)3 * H * dh;
  double maxerr = 0;
  std::vector<float> s(T);
  for (int p = 0; p < npairs; ++p) {
    const int b = pairs[p][0], hh = pairs[p][1];
    for (int q = 0; q < T; ++q) {
      const uint16_t* qp = &hq[((size_t)b * T + q) * ld + hh * dh];
      float mx = -1e30f;
      const int kend = causal ? q + 1 : T;
      for (int k = 0; k < kend; ++k) {
        const uint16_t* kp = &hq[((size_t)b * T + k) * ld + H * dh + hh * dh];
        float a = 0;
        for (int d = 0; d < dh; ++d) a += h2f(qp[d]) * h2f(kp[d]);
        s[k] = a / sqrtf((float)dh);
        mx = std::max(mx, s[k]);
      }
      double sum = 0;
      for (int k = 0; k < kend; ++k) { s[k] = expf(s[k] - mx); sum += s[k]; }
      for (int d = 0; d < dh; ++d) {
        double o = 0;
        for (int k = 0; k < kend; ++k) o += s[k] * h2f(hq[((size_t)b * T + k) * ld + 2 * H * dh + hh * dh + d]);
        o /= sum;
        maxerr = std::max(maxerr, fabs(o - bf2f(ho[((size_t)b * T + q) * (H * dh) + hh * dh + d])));
      }
    }
  }
  return maxerr;
}

// the comma-list mode: several head dimensions alternating in one process
static int compare_dhs(attn_fn attn, int B, int T, int H, const std::vector<int>& dhs) {
  const int n = (int)dhs.size(), rounds = 9, per = 20;
  std::vector<void*> dq(n), dout(n);
  hipStream_t st; CK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  int bad = 0;
  for (int i = 0; i < n; ++i) {
    const int dh = dhs[i];
    const size_t nq = (size_t)B * T * 3 * H * dh, no = (size_t)B * T * H * dh;
    std::vector<uint16_t> hq(nq), ho(no);
    unsigned r = 777u + (unsigned)dh;
    for (auto& v : hq) { r = r * 1664525u + 1013904223u; v = f2h((((int)(r >> 9) & 0xffff) / 32768.f - 1.f) * 1.5f); }
    CK(hipMalloc(&dq[i], nq * 2)); CK(hipMalloc(&dout[i], no * 2));
    CK(hipMemcpy(dq[i], hq.data(), nq * 2, hipMemcpyHostToDevice));
    if (attn(0, dq[i], dout[i], B, T, H, dh, 0, st)) { fprintf(stderr, "attention call failed at dh %d\n", dh); return 2; }
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(ho.data(), dout[i], no * 2, hipMemcpyDeviceToHost));
    const int pairs[1][2] = {{B - 1, H - 1}};  // the last head of the last sample: its fragments end where the buffer ends
    const double err = cpu_check(hq, ho, T, H, dh, 0, pairs, 1);
    printf("dh %d: max |err| vs fp32 CPU on the last (batch, head) pair %.4g\n", dh, err);
    bad |= !(err < 0.02);
  }
  if (bad) return 1;
  std::vector<std::vector<float>> med(n);
  for (int r = 0; r < rounds; ++r)
    for (int i = 0; i < n; ++i) {
      int rc = 0;  // a refused launch would be timed as a very fast kernel: every return code of the round counts
      for (int k = 0; k < 3; ++k) rc |= attn(0, dq[i], dout[i], B, T, H, dhs[i], 0, st);
      std::vector<float> t;
      for (int k = 0; k < per; ++k) {
        CK(hipEventRecord(e0, st)); rc |= attn(0, dq[i], dout[i], B, T, H, dhs[i], 0, st); CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1)); t.push_back(ms);
      }
      if (rc) { fprintf(stderr, "attention call failed at dh %d in round %d\n", dhs[i], r); return 2; }
      std::sort(t.begin(), t.end());
      med[i].push_back(t[t.size() / 2]);
    }
  double base = 0;
  for (int i = 0; i < n; ++i) {
    std::sort(med[i].begin(), med[i].end());
    const double m = med[i][med[i].size() / 2];
    const int dh = dhs[i], steps = (dh + 15) / 16 + 2 * ((dh + 31) / 32);
    const double fl = 4.0 * B * H * (double)T * T * dh;
    if (i == 0) base = m / steps;
    printf("attention B=%d T=%d H=%d dh=%d: median of %d round medians %.1f us (%.1f TFLOP/s on dh %d), spread %.1f .. %.1f us; %d MFMA steps per key block, "
           "time per step %.2f x dh %d's\n", B, T, H, dh, rounds, m * 1e3, fl / (m * 1e-3) / 1e12, dh, med[i].front() * 1e3, med[i].back() * 1e3, steps,
           m / steps / base, dhs[0]);
  }
  for (int i = 0; i < n; ++i) { CK(hipFree(dq[i])); CK(hipFree(dout[i])); }
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1)); CK(hipStreamDestroy(st));
  return 0;
}

int main(int argc, char** argv) {
  std::string self = argv[0];
  std::string dir = self.substr(0, self.find_last_of('/') == std::string::npos ? 0 : self.find_last_of('/'));
  void* h = dlopen(((dir.empty() ? std::string(".") : dir) + (getenv("CLIPX_LIB") ? std::string("/../clip-retrieval_amd/lib/") + getenv("CLIPX_LIB") : std::string("/../clip-retrieval_amd/lib/libclipx.so"))).c_str(), RTLD_NOW);
  if (!h) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
  attn_fn attn = (attn_fn)dlsym(h, "clipx_attention_dh_device");
  const int B = argc > 1 ? atoi(argv[1]) : 256, T = argc > 2 ? atoi(argv[2]) : 257, H = argc > 3 ? atoi(argv[3]) : 16;
  if (argc > 4 && strchr(argv[4], ',')) {
    std::vector<int> dhs;
    for (const char* p = argv[4]; p && *p;) {
      char* end;
      const long dh = strtol(p, &end, 10);
      if (end == p || (*end != ',' && *end != 0) || dh <= 0 || dh > 256) { fprintf(stderr, "bad head dimension list '%s'\n", argv[4]); return 2; }
      dhs.push_back((int)dh);
      p = *end ? end + 1 : nullptr;
    }
    return compare_dhs(attn, B, T, H, dhs);
  }
  const int dh = argc > 4 ? atoi(argv[4]) : 64, causal = argc > 5 ? atoi(argv[5]) : 0;
  const size_t ld = (size_t)3 * H * dh, nq = (size_t)B * T * ld, no = (size_t)B * T * H * dh;
  std::vector<uint16_t> hq(nq), ho(no);
  unsigned r = 777u;
  for (auto& v : hq) { r = r * 1664525u + 1013904223u; v = f2h((((int)(r >> 9) & 0xffff) / 32768.f - 1.f) * 1.5f); }
  void *dq, *dout;
  CK(hipMalloc(&dq, nq * 2)); CK(hipMalloc(&dout, no * 2));
  CK(hipMemcpy(dq, hq.data(), nq * 2, hipMemcpyHostToDevice));
  hipStream_t st; CK(hipStreamCreate(&st));
  if (attn(0, dq, dout, B, T, H, dh, causal, st)) { fprintf(stderr, "attention call failed\n"); return 2; }
  CK(hipStreamSynchronize(st));
  CK(hipMemcpy(ho.data(), dout, no * 2, hipMemcpyDeviceToHost));
  double maxerr = 0;
  const int pairs[3][2] = {{0, 0}, {B / 2, H - 1}, {B - 1, H / 2}};
  std::vector<float> s(T);
  for (auto& ph : pairs) {
    const int b = ph[0], hh = ph[1];
    for (int q = 0; q < T; ++q) {
      const uint16_t* qp = &hq[((size_t)b * T + q) * ld + hh * dh];
      float mx = -1e30f;
      const int kend = causal ? q + 1 : T;
      for (int k = 0; k < kend; ++k) {
        const uint16_t* kp = &hq[((size_t)b * T + k) * ld + H * dh + hh * dh];
        float a = 0;
        for (int d = 0; d < dh; ++d) a += h2f(qp[d]) * h2f(kp[d]);
        s[k] = a / sqrtf((float)dh);
        mx = std::max(mx, s[k]);
      }
      double sum = 0;
      for (int k = 0; k < kend; ++k) { s[k] = expf(s[k] - mx); sum += s[k]; }
      for (int d = 0; d < dh; ++d) {
        double o = 0;
        for (int k = 0; k < kend; ++k) o += s[k] * h2f(hq[((size_t)b * T + k) * ld + 2 * H * dh + hh * dh + d]);
        o /= sum;
        maxerr = std::max(maxerr, fabs(o - bf2f(ho[((size_t)b * T + q) * (H * dh) + hh * dh + d])));
      }
    }
  }
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::vector<float> ts;
  for (int i = 0; i < 12; ++i) {
    CK(hipEventRecord(e0, st)); attn(0, dq, dout, B, T, H, dh, causal, st); CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ts.push_back(ms);
  }
  std::sort(ts.begin(), ts.end());
  const double fl = 4.0 * B * H * (double)T * T * dh * (causal ? 0.5 : 1.0);
  printf("attention B=%d T=%d H=%d dh=%d causal=%d cfg=%s: median %.1f us (%.1f TFLOP/s), min %.1f us; max |err| vs fp32 CPU on 3 heads %.4g\n", B, T, H, dh,
         causal, getenv("CLIPX_ATTN_CFG") ? getenv("CLIPX_ATTN_CFG") : "-", ts[ts.size() / 2] * 1e3, fl / (ts[ts.size() / 2] * 1e-3) / 1e12, ts[0] * 1e3, maxerr);
  const int ab_cfg = argc > 6 ? atoi(argv[6]) : 0;
  if (ab_cfg == 19 && ((T + 31) / 32 != 19 || dh != 64 || causal)) {
    // the yardstick is instantiated at 19 key blocks only: anywhere else the library would run the default kernel under both names
    fprintf(stderr, "ab_cfg 19 (the RECOMP yardstick) exists for T = 577 .. 608, dh 64, not causal only: no A/B at T = %d dh = %d causal = %d\n", T, dh, causal);
    return 2;
  }
  if (ab_cfg > 0 && !(getenv("CLIPX_LIB") && strstr(getenv("CLIPX_LIB"), "ablate"))) {
    fprintf(stderr, "ab_cfg needs the tools library (CLIPX_LIB=libclipx_ablate.so): the product library has no A/B configurations\n");
    return 2;
  }
  if (ab_cfg > 0) {
    const int rounds = 9, per = 20;
    std::vector<float> med[2];
    std::vector<uint16_t> o2[2] = {std::vector<uint16_t>(no), std::vector<uint16_t>(no)};
    const std::string cfgs = std::to_string(ab_cfg);
    for (int r = 0; r < rounds; ++r)
      for (int c = 0; c < 2; ++c) {
        if (c) setenv("CLIPX_ATTN_CFG", cfgs.c_str(), 1); else unsetenv("CLIPX_ATTN_CFG");
        for (int i = 0; i < 3; ++i) if (attn(0, dq, dout, B, T, H, dh, causal, st)) { fprintf(stderr, "attention call failed (cfg %d)\n", c ? ab_cfg : 0); return 2; }
        std::vector<float> t;
        for (int i = 0; i < per; ++i) {
          CK(hipEventRecord(e0, st)); attn(0, dq, dout, B, T, H, dh, causal, st); CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
          float ms; CK(hipEventElapsedTime(&ms, e0, e1)); t.push_back(ms);
        }
        std::sort(t.begin(), t.end());
        med[c].push_back(t[t.size() / 2]);
        if (r == 0) CK(hipMemcpy(o2[c].data(), dout, no * 2, hipMemcpyDeviceToHost));
      }
    unsetenv("CLIPX_ATTN_CFG");
    double dmax = 0; size_t ndiff = 0;
    for (size_t i = 0; i < no; ++i) { const double d = fabs(bf2f(o2[0][i]) - bf2f(o2[1][i])); dmax = std::max(dmax, d); ndiff += o2[0][i] != o2[1][i]; }
    for (int c = 0; c < 2; ++c) {
      std::sort(med[c].begin(), med[c].end());
      const double m = med[c][med[c].size() / 2];
      printf("  A/B %s: median of %d round medians %.1f us (%.1f TFLOP/s), spread %.1f .. %.1f us\n", c ? ("cfg " + cfgs).c_str() : "default",
             rounds, m * 1e3, fl / (m * 1e-3) / 1e12, med[c].front() * 1e3, med[c].back() * 1e3);
    }
    printf("  A/B outputs: max |default - cfg %d| = %.4g, %zu of %zu bf16 values differ\n", ab_cfg, dmax, ndiff, no);
    if (dmax > 0.02) return 1;
  }
  typedef int (*dbg_fn)(long long*, int);
  dbg_fn dbgf = (dbg_fn)dlsym(h, "clipx_dbg_attn_phase");
  if (dbgf && getenv("CLIPX_ATTN_CFG") && atoi(getenv("CLIPX_ATTN_CFG")) == 9) {
    const int nw = std::min(B * H, 2048) * 3;
    std::vector<long long> ph((size_t)nw * 4);
    if (!dbgf(ph.data(), nw * 4)) {
      double s4[4] = {0, 0, 0, 0};
      for (int i = 0; i < nw; ++i) for (int j = 0; j < 4; ++j) s4[j] += ph[(size_t)i * 4 + j] / (double)nw;
      printf("  phases, shader cycles per wave (3 query blocks): staging %.0f | S + max %.0f | exp + PV %.0f | store %.0f\n", s4[0], s4[1], s4[2], s4[3]);
    }
  }
  dbgf = (dbg_fn)dlsym(h, "clipx_dbg_attn_pk_phase");  // each kernel file owns its phase array (no relocatable device code)
  if (dbgf && getenv("CLIPX_ATTN_PK_TIMER") && atoi(getenv("CLIPX_ATTN_PK_TIMER"))) {
    // persistent kernel (attention_pk_kernel): per wave index, averaged over the workgroups, shader cycles of the LAST launch
    const int nwg = std::min(B * H, 256);
    std::vector<long long> ph((size_t)nwg * 6 * 4);
    if (!dbgf(ph.data(), nwg * 6 * 4)) {
      for (int w = 0; w < 6; ++w) {
        double s4[4] = {0, 0, 0, 0};
        for (int g = 0; g < nwg; ++g) for (int j = 0; j < 4; ++j) s4[j] += ph[((size_t)g * 6 + w) * 4 + j] / (double)nwg;
        const double pairs = (double)B * H / nwg;
        printf("  wave %d, shader cycles per pair: wait + barrier %.0f | DMA issue %.0f | S %.0f | exp + PV + out %.0f | sum %.0f\n", w,
               s4[0] / pairs, s4[1] / pairs, s4[2] / pairs, s4[3] / pairs, (s4[0] + s4[1] + s4[2] + s4[3]) / pairs);
      }
    }
  }
  return maxerr < 0.02 ? 0 : 1;
}
