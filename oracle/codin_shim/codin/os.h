/* codin/os.h -- stand-in, written for this project (see codin.h).
 * ASSUMPTIONS about the real codin: raytracer.c:6, scene.c:4 and denoiser.c:6 include it for processor_yield(), which
 * this stand-in declares in thread.h (assumption T2); nothing else of it is used by the sources served here. */
#ifndef CODIN_SHIM_OS_H
#define CODIN_SHIM_OS_H
#include "thread.h"
#endif
