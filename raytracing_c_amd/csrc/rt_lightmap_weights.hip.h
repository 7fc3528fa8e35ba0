// rt_lightmap_weights.hip.h -- the ONE text of the lightmap rasteriser's acceptance test (raytracer.c:733-747), shared by
// lightmap_bake's kernels (rt_kernels.hip) and the HDR lightmap's texel list (rt_lightmap.hip).
#pragma once

// barycentric weights of texel (x, y) for the UV triangle (p0, p1, p2), raytracer.c:733-747
__device__ __forceinline__ bool lightmap_weights(float p0x, float p0y, float p1x, float p1y, float p2x, float p2y,
                                                 int x, int y, float &w0, float &w1, float &w2) {
  float denom = (p1y - p2y) * (p0x - p2x) + (p2x - p1x) * (p0y - p2y);
  float px = (float)x, py = (float)y;
  w0 = ((p1y - p2y) * (px - p2x) + (p2x - p1x) * (py - p2y)) / denom;
  w1 = ((p2y - p0y) * (px - p2x) + (p0x - p2x) * (py - p2y)) / denom;
  w2 = 1.0f - w0 - w1;
  return w0 >= -RT_EPS && w1 >= -RT_EPS && w2 >= -RT_EPS;
}

__device__ __forceinline__ float min3f(float a, float b, float c) { float m = b < c ? b : c; return a < m ? a : m; }
__device__ __forceinline__ float max3f(float a, float b, float c) { float m = b > c ? b : c; return a > m ? a : m; }
