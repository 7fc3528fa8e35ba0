// Round 13's candidates for the short forms of the environment lookup and the normalisations (rt_dev.hip.h: atan_pos_dev, asin_dev,
// inv_sqrt_exact, sqrt_dev, the background's coordinates), each against the rt_math.h function over all 2^32 bit patterns: which
// of the square root's two one-ulp corrections are needed, whether the quotient of the arctangent needs the Newton step on its
// reciprocal and how its infinite denominator is guarded, whether the root's class test is needed, whether the negative wrap of a
// texture coordinate ever fires.  Results: profiles/r13_env_forms.md.  The shipped forms are swept by tests/test_gpu_env_forms.py.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -std=c++17 -Iinclude tools/exp/env_forms_test.hip -o tools/exp/env_forms_test
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "rt_math.h"

__device__ __forceinline__ int as_i(float f) { return __float_as_int(f); }
__device__ __forceinline__ float as_f(int i) { return __int_as_float(i); }

__device__ __forceinline__ float rcp_exact(float x) {
  float xs = x * 0x1p24f;
  float y = __builtin_amdgcn_rcpf(xs);
  float e = __builtin_fmaf(-xs, y, 1.0f);
  float z = __builtin_fmaf(e, y, y);
  return __builtin_amdgcn_div_fixupf(z, xs, 1.0f) * 0x1p24f;
}

template <bool DOWN, bool UP>
__device__ __forceinline__ float sqrt_core(float x, float &raw) {
  const float r = __builtin_amdgcn_sqrtf(x);
  raw = r;
  float res = r;
  if (DOWN) { const float dn = as_f(as_i(r) - 1); const float vp = __builtin_fmaf(-dn, r, x); res = (vp <= 0.0f) ? dn : res; }
  if (UP) { const float up = as_f(as_i(r) + 1); const float vs = __builtin_fmaf(-up, r, x); res = (vs > 0.0f) ? up : res; }
  return res;
}

template <bool DOWN, bool UP>
__device__ __forceinline__ float asin_dev(float x) {
  float a = rt_absf(x);
  if (a > 1.0f) a = 1.0f;
  int big = a > 0.5f;
  float z, w, raw;
  if (big) { z = 0.5f * (1.0f - a); w = sqrt_core<DOWN, UP>(z, raw); } else { w = a; z = a * a; }
  float p = rt_fmaf(rt_fmaf(rt_fmaf(rt_fmaf(4.2163199048E-2f, z, 2.4181311049E-2f), z, 4.5470025998E-2f), z, 7.4953002686E-2f),
                    z, 1.6666752422E-1f);
  p = rt_fmaf(p * z, w, w);
  if (big) p = 1.5707963267948966192f - (p + p);
  return x < 0.0f ? -p : p;
}

// inverse sqrt variants
__device__ __forceinline__ float inv_sqrt_v0(float s) {
  const float r = rt_sqrtf(s);
  const float y = __builtin_amdgcn_rcpf(r);
  const float e = __builtin_fmaf(-r, y, 1.0f);
  const float z = __builtin_fmaf(e, y, y);
  return __builtin_amdgcn_div_fixupf(z, r, 1.0f);
}
template <bool DOWN, bool UP>
__device__ __forceinline__ float inv_sqrt_v1(float s) {
  const bool sc = s < 0x1p-96f;
  const float xs = s * (sc ? 0x1p32f : 1.0f);
  float raw;
  const float r = sqrt_core<DOWN, UP>(xs, raw);
  const float y = __builtin_amdgcn_rcpf(r);
  const float e = __builtin_fmaf(-r, y, 1.0f);
  float z = __builtin_fmaf(e, y, y);
  z = __builtin_amdgcn_div_fixupf(z, raw, 1.0f);
  return z * (sc ? 0x1p16f : 1.0f);
}
template <bool CLASSFIX>
__device__ __forceinline__ float sqrt_dev(float s) {
  const bool sc = s < 0x1p-96f;
  const float xs = s * (sc ? 0x1p32f : 1.0f);
  float raw;
  float r = sqrt_core<true, true>(xs, raw);
  r = r * (sc ? 0x1p-16f : 1.0f);
  if (CLASSFIX) r = (xs == 0.0f || xs == RT_INF) ? xs : r;
  return r;
}

// atan variants.  GUARD 0: none, 1: min(den, 2^100), 2: div_fixup
template <bool NEWTON, int GUARD>
__device__ __forceinline__ float atan_pos_dev(float a) {
  const bool big = a > 2.414213562373095f;
  const bool mid = a > 0.4142135623730950f;
  const float num = big ? -1.0f : a - 1.0f;
  float den = big ? a : a + 1.0f;
  if (GUARD == 1) den = __builtin_fminf(den, 0x1p100f);
  const float yb = big ? 1.5707963267948966192f : (mid ? 0.7853981633974483096f : 0.0f);
  float y = __builtin_amdgcn_rcpf(den);
  if (NEWTON) { const float e = __builtin_fmaf(-den, y, 1.0f); y = __builtin_fmaf(e, y, y); }
  const float q0 = num * y;
  const float r = __builtin_fmaf(-den, q0, num);
  float q = __builtin_fmaf(r, y, q0);
  if (GUARD == 2) q = __builtin_amdgcn_div_fixupf(q, den, num);
  const float t = mid ? q : a;
  const float z = t * t;
  const float p = rt_fmaf(rt_fmaf(rt_fmaf(8.05374449538e-2f, z, -1.38776856032E-1f), z, 1.99777106478E-1f), z, -3.33329491539E-1f);
  return yb + rt_fmaf(p * z, t, t);
}

template <bool WRAP>
__device__ __forceinline__ float tex_wrap_fract(float tx) {
  if (WRAP && tx < 0) tx += (float)(-(int)tx + 1);
  return rt_fractf(tx);
}
__device__ __forceinline__ float bg_u(float t) { return rt_madd(t, 1.0f / (2.0f * RT_PI), 0.5f); }
__device__ __forceinline__ float bg_v(float t) { return rt_madd(-t, 1.0f / RT_PI, 0.5f); }

__device__ __forceinline__ bool same_bits(float w, float g, bool &strict) {
  const uint32_t a = __float_as_uint(w), b = __float_as_uint(g);
  strict = a == b;
  const bool an = (a & 0x7FFFFFFFu) > 0x7F800000u, bn = (b & 0x7FFFFFFFu) > 0x7F800000u;
  return an ? bn : (a == b);
}

// counts[0] differing (NaN == NaN), [1] first + 1, [2] differing bit-strict, [3] in-domain patterns
template <int ID>
__global__ void sweep(unsigned long long *counts) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t bad = 0, first = 0, sbad = 0, n = 0;
  for (uint32_t k = 0; k < 256u; k++) {
    const uint32_t b = tid * 256u + k;
    const float x = __uint_as_float(b);
    float w = 0, g = 0;
    bool in = true;
    switch (ID) {
    case 0: w = rt_atanf_pos(x); g = atan_pos_dev<true, 1>(x); break;
    case 1: w = rt_atanf_pos(x); g = atan_pos_dev<false, 1>(x); break;
    case 2: w = rt_atanf_pos(x); g = atan_pos_dev<true, 0>(x); break;
    case 3: w = rt_atanf_pos(x); g = atan_pos_dev<true, 2>(x); break;
    case 4: w = rt_atanf_pos(x); g = atan_pos_dev<false, 2>(x); break;
    case 10: w = rt_asinf(x); g = asin_dev<true, true>(x); break;
    case 11: w = rt_asinf(x); g = asin_dev<true, false>(x); break;
    case 12: w = rt_asinf(x); g = asin_dev<false, true>(x); break;
    case 13: w = rt_asinf(x); g = asin_dev<false, false>(x); break;
    case 20: w = rcp_exact(rt_sqrtf(x)); g = inv_sqrt_v0(x); break;
    case 21: w = rcp_exact(rt_sqrtf(x)); g = inv_sqrt_v1<true, true>(x); break;
    case 22: w = rcp_exact(rt_sqrtf(x)); g = inv_sqrt_v1<true, false>(x); break;
    case 23: w = rcp_exact(rt_sqrtf(x)); g = inv_sqrt_v1<false, true>(x); break;
    case 24: w = rcp_exact(rt_sqrtf(x)); g = inv_sqrt_v1<false, false>(x); break;
    case 25: w = 1.0f / rt_sqrtf(x); g = inv_sqrt_v1<true, true>(x); break;
    case 30: w = rt_sqrtf(x); g = sqrt_dev<true>(x); break;
    case 31: w = rt_sqrtf(x); g = sqrt_dev<false>(x); break;
    case 40: in = !(__builtin_fabsf(x) > RT_PI); w = tex_wrap_fract<true>(bg_u(x)); g = tex_wrap_fract<false>(bg_u(x)); break;
    case 41: in = !(__builtin_fabsf(x) > 1.5707963267948966192f); w = tex_wrap_fract<true>(bg_v(x)); g = tex_wrap_fract<false>(bg_v(x)); break;
    }
    if (!in) continue;
    n += 1;
    bool strict;
    if (!same_bits(w, g, strict)) { bad += 1; if (!first) first = b + 1u; }
    if (!strict) sbad += 1;
  }
  if (bad) atomicAdd(&counts[0], (unsigned long long)bad);
  if (first) atomicMax(&counts[1], (unsigned long long)first);
  if (sbad) atomicAdd(&counts[2], (unsigned long long)sbad);
  atomicAdd(&counts[3], (unsigned long long)n);
}

template <int ID>
static int run(const char *name, unsigned long long *d) {
  unsigned long long h[4] = {0, 0, 0, 0};
  if (hipMemset(d, 0, sizeof h) != hipSuccess) return 1;
  hipLaunchKernelGGL(sweep<ID>, dim3(65536), dim3(256), 0, 0, d);
  if (hipDeviceSynchronize() != hipSuccess) { printf("%s: sync failed\n", name); return 1; }
  if (hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  printf("%-40s differ %llu  first %#llx  strict %llu  n %llu\n", name, h[0], h[1] ? h[1] - 1 : 0ull, h[2], h[3]);
  fflush(stdout);
  return 0;
}

int main() {
  unsigned long long *d;
  if (hipMalloc(&d, 32) != hipSuccess) { printf("no device\n"); return 1; }
  int rc = 0;
#define R(ID, NAME) if (!rc) rc = run<ID>(NAME, d)
  R(0, "atan newton min");
  R(1, "atan short min");
  R(2, "atan newton noguard");
  R(3, "atan newton fixup");
  R(4, "atan short fixup");
  R(10, "asin down up");
  R(11, "asin down");
  R(12, "asin up");
  R(13, "asin none");
  R(20, "invsqrt v0 (rt_sqrtf + noscale rcp)");
  R(21, "invsqrt v1 down up");
  R(22, "invsqrt v1 down");
  R(23, "invsqrt v1 up");
  R(24, "invsqrt v1 none");
  R(25, "invsqrt v1 down up vs 1/sqrt");
  R(30, "sqrt_dev classfix");
  R(31, "sqrt_dev no classfix");
  R(40, "u wrap");
  R(41, "v wrap");
  (void)hipFree(d);
  return rc;
}
