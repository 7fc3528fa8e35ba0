// Micro-benchmark: what the LDS array of a CU pays for the path kernel's sample adds -- ds_add_u64 without return, three per
// sample (24-byte pixels of a wave's accumulator tile, tile_add_sample) -- with 64, 16, 4 or 1 lanes of a wave on one address,
// and what such adds cost a neighbour's node reads.  One 1024-thread workgroup per CU, 16 waves, the path kernel's LDS size
// (node image + 16 accumulator tiles), as in lds_node_bench.hip.
//   all16   every wave adds                                               -> cycles of the CU per add instruction
//   add8    waves 0-1 of every SIMD add, the others have left             (the adders of `mixed`, alone)
//   read8   waves 2-3 of every SIMD do full node blocks (12 x ds_read_b128 on a random node per lane), the others have left
//   mixed   8 adders beside 8 readers: the TIMED role runs a fixed number of rounds, the other role runs until the timed waves
//           are done (a flag in LDS, looked at every 16 rounds), so the timed role is under contention from start to end
// Times are per wave and round (s_memrealtime, 100 MHz), averaged over the timed waves of all CUs.
// hipcc --offload-arch=gfx950 -O3 lds_add_bench.hip -o lds_add_bench && ./lds_add_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
#define N_NODES 585
#define STRIDE_F 52                      // 208 bytes per node
#define NODE_BYTES (N_NODES * STRIDE_F * 4)
#define TILE_BYTES (64 * 24)             // 64 pixels x 3 u64
#define FLAG_OFF (NODE_BYTES + 16 * TILE_BYTES)
#define SMEM_BYTES (FLAG_OFF + 16)
#define N_CU 256
#define CLOCK_GHZ 2.4

enum { MODE_ALL16, MODE_ADD8, MODE_READ8, MODE_MIXED_TIME_ADD, MODE_MIXED_TIME_READ };

__device__ __forceinline__ uint32_t pcg(uint32_t v) {
  uint32_t s = v * 747796405u + 2891336453u;
  uint32_t w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
  return (w >> 22u) ^ w;
}

// `lanes`: lanes of a wave per address (64, 16, 4, 1).  ticks[cu * 16 + wave] = s_memrealtime ticks of the wave's timed loop, 0 for
// a wave that was not timed.
__global__ __launch_bounds__(1024) void bench(int mode, int lanes, int iters, unsigned long long *ticks, float *out) {
  extern __shared__ float smem[];
  for (int i = threadIdx.x; i < FLAG_OFF / 4 + 4; i += 1024) smem[i] = i < NODE_BYTES / 4 ? 1.0f + (float)(i & 7) : 0.0f;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool adder = mode == MODE_ALL16 || ((wave >> 2) & 1) == 0;        // (waves go to SIMDs round robin: 2 adders + 2 readers each)
  const bool mixed = mode == MODE_MIXED_TIME_ADD || mode == MODE_MIXED_TIME_READ;
  if ((mode == MODE_ADD8 && !adder) || (mode == MODE_READ8 && adder)) return;
  const bool timed = !mixed || (adder == (mode == MODE_MIXED_TIME_ADD));
  volatile uint32_t *flag = reinterpret_cast<volatile uint32_t *>(reinterpret_cast<char *>(smem) + FLAG_OFF);
  uint32_t rng = pcg(blockIdx.x * 1024u + threadIdx.x + 1u);
  float acc = 0.0f;
  int pixel = lane / lanes;
  asm volatile("" : "+v"(pixel));        // a per-lane address the compiler cannot prove wave-uniform, as in the kernel: plain ds_add_u64
  unsigned long long *ap = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(smem) + NODE_BYTES + wave * TILE_BYTES) + pixel * 3;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < (timed ? iters : iters * 64); it++) {        // (the bound of the untimed role: no wave can wait for ever)
    rng = pcg(rng);
    if (adder) {
      const unsigned long long v = ((unsigned long long)rng << 16) | 1ull;
      atomicAdd(ap + 0, v);
      atomicAdd(ap + 1, v + 1ull);
      atomicAdd(ap + 2, v + 2ull);
    } else {
      const float4 *q = reinterpret_cast<const float4 *>(smem + (rng % N_NODES) * STRIDE_F);
#pragma unroll
      for (int k = 0; k < 12; k++) { float4 v = q[k]; acc += v.x + v.y + v.z + v.w; }
    }
    if (!timed && (it & 15) == 15 && *flag >= 8u) break;
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
  if (timed && mixed && lane == 0) atomicAdd(const_cast<uint32_t *>(flag), 1u);
  if (lane == 0) ticks[blockIdx.x * 16 + wave] = timed ? t1 - t0 : 0ull;
  if (acc == 12345.678f) out[0] = acc;
}

static double run(int mode, int lanes, unsigned long long *d_ticks, float *out) {
  const int iters = 20000;
  static unsigned long long h[N_CU * 16];
  for (int pass = 0; pass < 2; pass++) {                // (the first pass warms up)
    CHECK(hipMemset(d_ticks, 0, sizeof h));
    hipLaunchKernelGGL(bench, dim3(N_CU), dim3(1024), SMEM_BYTES, 0, mode, lanes, pass ? iters : 200, d_ticks, out);
    CHECK(hipDeviceSynchronize());
  }
  CHECK(hipMemcpy(h, d_ticks, sizeof h, hipMemcpyDeviceToHost));
  double sum = 0; int n = 0;
  for (int i = 0; i < N_CU * 16; i++) if (h[i]) { sum += (double)h[i]; n++; }
  return n ? sum / n * 10.0 / iters : 0.0;              // ns per wave and round
}

int main() {
  float *out; unsigned long long *d_ticks;
  CHECK(hipMalloc(&out, 64));
  CHECK(hipMalloc(&d_ticks, N_CU * 16 * sizeof(unsigned long long)));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&bench), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  const double rd = run(MODE_READ8, 64, d_ticks, out);
  printf("read8 alone: %8.1f ns per node block (12 x ds_read_b128) and wave = %6.0f cycles\n", rd, rd * CLOCK_GHZ);
  double all1 = 0;
  const int L[4] = {1, 4, 16, 64};
  for (int i = 0; i < 4; i++) {
    const double a16 = run(MODE_ALL16, L[i], d_ticks, out), a8 = run(MODE_ADD8, L[i], d_ticks, out);
    const double ma = run(MODE_MIXED_TIME_ADD, L[i], d_ticks, out), mr = run(MODE_MIXED_TIME_READ, L[i], d_ticks, out);
    if (i == 0) all1 = a16;
    // the CU's LDS array serves 16 waves x 3 adds in a16 ns: cycles of the array per add instruction, and per lane beyond the
    // first on an address (against the conflict-free case)
    const double cyc = a16 * CLOCK_GHZ / (16.0 * 3.0);
    const double per_lane = L[i] > 1 ? (a16 - all1) * CLOCK_GHZ / (16.0 * 3.0 * (L[i] - 1)) : 0.0;
    printf("%2d lanes/address: all16 %8.1f ns/round = %6.1f CU cycles per ds_add_u64, %5.2f per extra same-address lane | add8 alone %8.1f"
           " | mixed: adders %8.1f, readers %8.1f ns (x%.2f of read8 alone)\n", L[i], a16, cyc, per_lane, a8, ma, mr, mr / rd);
  }
  return 0;
}
