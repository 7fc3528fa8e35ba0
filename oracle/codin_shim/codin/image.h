/* codin/image.h -- stand-in, written for this project (see codin.h).
 * ASSUMPTIONS about the real codin, with the reference line that uses each:
 *   I1  Image has components, pixel_type, width, stride, height (isize) and pixels (a byte slice); the layout is the
 *       one of include/rt_types.h, which IS this project's ABI                       raytracer.c:606-607,714-716,723-724
 *   I2  PT_u8 names the 8-bit pixel type                                            raytracer.c:723
 *   I3  texel c of pixel (x, y) is pixels[components * (x + y * stride) + c]         raytracer.c:714, denoiser.c:24
 */
#ifndef CODIN_SHIM_IMAGE_H
#define CODIN_SHIM_IMAGE_H
#include "codin.h"
#endif
