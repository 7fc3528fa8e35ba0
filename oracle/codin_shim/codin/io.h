/* codin/io.h -- stand-in, written for this project (see codin.h).
 * ASSUMPTIONS about the real codin, with the reference line that uses each:
 *   W1  a Writer is passed by pointer; write_bytes(w, bytes) appends a byte slice, write_any(w, &value) appends the
 *       bytes of the value                                                            scene.c:18,26,32-33
 * scene_save_writer is compiled but not exported by the harness. */
#ifndef CODIN_SHIM_IO_H
#define CODIN_SHIM_IO_H
#include "codin.h"
static inline void write_bytes(Writer const *w, Byte_Slice bytes) { w->proc(w->user, bytes); }
#define write_any(w, p) write_bytes((w), (Byte_Slice){ .data = (byte *)(p), .len = size_of(*(p)) })
#endif
