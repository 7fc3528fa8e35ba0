/* codin/sync.h -- stand-in, written for this project (see codin.h).
 * ASSUMPTIONS about the real codin: none of its names is used by the sources this stand-in serves; scene.h:6 only
 * includes it (the atomics of raytracer.h:48 and scene.c:248-257 are C11 <stdatomic.h>). */
#ifndef CODIN_SHIM_SYNC_H
#define CODIN_SHIM_SYNC_H
#include "codin.h"
#endif
