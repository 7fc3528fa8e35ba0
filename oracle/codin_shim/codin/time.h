/* codin/time.h -- stand-in, written for this project (see codin.h).
 * ASSUMPTIONS about the real codin, with the reference line that uses each:
 *   C1  time_now() returns an integer clock value that converts to u32               raytracer.c:597
 * THIS STAND-IN returns the value the harness sets (codin_shim_time), so `random_state = time_now()` becomes the frame
 * seed exactly as ORACLE_LITERAL defines it (oracle/oracle.h). */
#ifndef CODIN_SHIM_TIME_H
#define CODIN_SHIM_TIME_H
#include "codin.h"
static i64 codin_shim_time;
static inline i64 time_now(void) { return codin_shim_time; }
#endif
