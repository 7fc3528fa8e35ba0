/* Sizes and field offsets of the HDR-lightmap structs of include/rt_hip.h, for tests/test_lightmap_hdr_cpu.py: "name value" per line. */
#include <stddef.h>
#include <stdio.h>

#include "rt_hip.h"

#define SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  SIZE(RT_Lightmap_Texel);
  OFF(RT_Lightmap_Texel, origin); OFF(RT_Lightmap_Texel, texel); OFF(RT_Lightmap_Texel, normal); OFF(RT_Lightmap_Texel, triangle);
  SIZE(RT_Lightmap_Params);
  OFF(RT_Lightmap_Params, width); OFF(RT_Lightmap_Params, height); OFF(RT_Lightmap_Params, samples);
  OFF(RT_Lightmap_Params, sample_first); OFF(RT_Lightmap_Params, sample_count); OFF(RT_Lightmap_Params, max_bounces);
  OFF(RT_Lightmap_Params, seed); OFF(RT_Lightmap_Params, scale);
  printf("RT_LIGHTMAP_MAX_TEXELS %lld\n", (long long)RT_LIGHTMAP_MAX_TEXELS);
  printf("RT_LIGHTMAP_MAX_PATHS %lld\n", (long long)RT_LIGHTMAP_MAX_PATHS);
  printf("RT_LIGHTMAP_MAX_PASSES %d\n", RT_LIGHTMAP_MAX_PASSES);
  printf("RT_LIGHTMAP_SLICE %lld\n", (long long)RT_LIGHTMAP_SLICE);
  return 0;
}
