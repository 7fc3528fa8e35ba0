/* Sizes and field offsets of the light-probe structs of include/rt_hip.h, for tests/test_probes_cpu.py: "name value" per line. */
#include <stddef.h>
#include <stdio.h>

#include "rt_hip.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  SIZE(RT_Probe_Sample);
  OFF(RT_Probe_Sample, radiance); OFF(RT_Probe_Sample, t); OFF(RT_Probe_Sample, direction); OFF(RT_Probe_Sample, pad);
  SIZE(RT_Probe_Params);
  OFF(RT_Probe_Params, samples); OFF(RT_Probe_Params, sample_first); OFF(RT_Probe_Params, sample_count);
  OFF(RT_Probe_Params, max_bounces); OFF(RT_Probe_Params, seed); OFF(RT_Probe_Params, probe_first);
  printf("RT_PROBE_COEFFS %d\n", RT_PROBE_COEFFS);
  printf("RT_PROBE_MAX_PATHS %lld\n", (long long)RT_PROBE_MAX_PATHS);
  printf("RT_PROBE_SLICE %lld\n", (long long)RT_PROBE_SLICE);
  return 0;
}
