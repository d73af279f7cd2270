// runtime.hip — what every other file of the library calls and nothing that launches model work: the error text, the
// version / arithmetic strings, the kernel timer, the deterministic-mode flag, the library-owned scratch and the
// stream-capture query (all declared in common.h).
#include "common.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <vector>

// ------------------------------------------------------------------ error text
static thread_local char g_err[512] = "";
void ps_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* ps_last_error(void) { return g_err; }
extern "C" const char* ps_version(void) { return "prodsearch_hip 0.1 (gfx950, fp32 MFMA)"; }
// what the step computes in (bench.py's `dtype`): everything is fp32 in and out; products run on the fp32 MFMA or, where the
// bf16x3 form is enabled (ps_gemm_x3_config, the fused per-replica kernels), as exact three-way bf16 splits of both fp32
// operands — six bf16 MFMAs per product step, fp32 accumulation, the fp32 MFMA's accuracy
extern "C" const char* ps_arith_info(void) {
  // (the SPLIT is exact — hi + mid + lo carry all 24 mantissa bits; the PRODUCT keeps six of the nine cross terms and drops those
  // below 2^-24 of the leading one: fp32-GRADE, 1.1e-7 of sum |a b| against fp64, the fp32 MFMA's own 1.13e-7 — not "exact")
  return gemm_x3_on() ? "f32 (fp32 MFMA and VALU; wide products, the fused per-replica kernels and grouped weight gradients as fp32-grade "
                        "bf16x3 products: exact 3-way bf16 split of both fp32 operands, 6 of the 9 cross products as bf16 MFMAs per step, "
                        "fp32 accumulation)"
                      : "f32 (fp32 MFMA and VALU)";
}

// ------------------------------------------------------------------ kernel timer (common.h)
static struct KTimer {
  char tag[32];
  bool armed, open;
  std::vector<hipEvent_t> e0, e1;
  int n, cap;
} g_kt = {"", false, false, {}, {}, 0, 0};
const char* ps_ktimer_tag() { return g_kt.armed ? g_kt.tag : nullptr; }
void ps_ktimer_scope(bool open) { g_kt.open = open && g_kt.armed; }
bool ps_ktimer_take(hipEvent_t* e0, hipEvent_t* e1) {
  if (!g_kt.open) return false;
  g_kt.open = false;                                              // one launch per scope
  if (g_kt.n >= g_kt.cap) return false;
  *e0 = g_kt.e0[g_kt.n]; *e1 = g_kt.e1[g_kt.n]; ++g_kt.n;
  return true;
}
extern "C" int ps_ktimer_arm(const char* tag, int32_t max_samples) {
  g_kt.armed = false; g_kt.open = false;
  g_kt.n = 0;
  if (!tag || !*tag || max_samples <= 0) return PS_OK;            // disarm
  PS_REQUIRE(strlen(tag) < sizeof(g_kt.tag), "ktimer: tag too long");
  while ((int)g_kt.e0.size() < max_samples) {
    hipEvent_t a, b;
    PS_CHECK_HIP(hipEventCreate(&a));
    PS_CHECK_HIP(hipEventCreate(&b));
    g_kt.e0.push_back(a); g_kt.e1.push_back(b);
  }
  g_kt.cap = max_samples;
  strcpy(g_kt.tag, tag);
  g_kt.armed = true;
  return PS_OK;
}
// average / min duration (us) of the launches bracketed since ps_ktimer_arm; synchronises the device; disarms
extern "C" int ps_ktimer_read(double* avg_us, double* min_us, int32_t* count) {
  PS_REQUIRE(avg_us && count, "ktimer: null argument");
  g_kt.armed = false; g_kt.open = false;
  PS_CHECK_HIP(hipDeviceSynchronize());
  double sum = 0, mn = 1e30;
  for (int i = 0; i < g_kt.n; ++i) {
    float ms = 0.f;
    PS_CHECK_HIP(hipEventElapsedTime(&ms, g_kt.e0[i], g_kt.e1[i]));
    sum += ms * 1e3; mn = ms * 1e3 < mn ? ms * 1e3 : mn;
  }
  *count = g_kt.n;
  *avg_us = g_kt.n ? sum / g_kt.n : 0.0;
  if (min_us) *min_us = g_kt.n ? mn : 0.0;
  g_kt.n = 0;
  return PS_OK;
}

// ---- deterministic mode (PS_DETERMINISTIC=1 or ps_set_deterministic): see common.h / DESIGN.md 5e
static int& det_slot() {
  static int v = ps_env_int("PS_DETERMINISTIC", 0);
  return v;
}
bool ps_deterministic() { return det_slot() != 0; }
extern "C" int ps_set_deterministic(int on) {
  const int old = det_slot();
  if (on >= 0) det_slot() = on ? 1 : 0;          // negative: query only
  return old;
}
bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
  return cs != hipStreamCaptureStatusNone;
}
float* ps_det_scratch(int slot, size_t floats, hipStream_t st) {
  static float* buf[PS_MAX_DEVICES][3];
  static size_t cap[PS_MAX_DEVICES][3];
  static std::mutex mu;
  int dev = 0;
  if (slot < 0 || slot > 2) return nullptr;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= PS_MAX_DEVICES) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lock(mu);
  if (cap[dev][slot] < floats) {
    if (stream_capturing(st)) return nullptr;
    (void)hipStreamSynchronize(st);                      // the old buffer may still be read by a queued launch
    if (buf[dev][slot]) (void)hipFree(buf[dev][slot]);
    buf[dev][slot] = nullptr; cap[dev][slot] = 0;
    const size_t want = floats + floats / 4;
    if (hipMalloc((void**)&buf[dev][slot], want * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    cap[dev][slot] = want;
  }
  return buf[dev][slot];
}
