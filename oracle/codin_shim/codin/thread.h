/* codin/thread.h -- stand-in, written for this project (see codin.h).
 * ASSUMPTIONS about the real codin, with the reference line that uses each:
 *   T1  thread_create(proc, arg, stack, tls) starts proc(arg) on another thread; Thread_Proc is void (*)(rawptr);
 *       THREAD_STACK_DEFAULT / THREAD_TLS_DEFAULT are plain constants                 scene.c:278, denoiser.c:141
 *   T2  processor_yield() lets other threads run                                      scene.c:284,298,304, raytracer.c:792
 * THIS STAND-IN is cooperative and single-threaded: thread_create() queues the procedure and processor_yield() runs
 * the queued procedures inline, one per call.  The builder's workers write disjoint nodes and leaf groups chosen by
 * index (scene.c:319,398,412), so the built Scene does not depend on which thread runs which task. */
#ifndef CODIN_SHIM_THREAD_H
#define CODIN_SHIM_THREAD_H
#include "codin.h"

typedef void (*Thread_Proc)(rawptr);
#define THREAD_STACK_DEFAULT 0
#define THREAD_TLS_DEFAULT   0

#define CODIN_SHIM_MAX_THREADS 64
typedef struct { Thread_Proc proc; rawptr arg; } Codin_Shim_Thread;
static Codin_Shim_Thread codin_shim_threads[CODIN_SHIM_MAX_THREADS];
static int               codin_shim_n_threads;

static inline void thread_create(Thread_Proc proc, rawptr arg, isize stack, isize tls) {
  (void)stack; (void)tls;
  if (codin_shim_n_threads >= CODIN_SHIM_MAX_THREADS) codin_shim_panic("too many threads", __FILE__, __LINE__);
  codin_shim_threads[codin_shim_n_threads].proc = proc;
  codin_shim_threads[codin_shim_n_threads].arg  = arg;
  codin_shim_n_threads += 1;
}

static inline void processor_yield(void) {
  if (codin_shim_n_threads == 0) codin_shim_panic("processor_yield with nothing left to run: the caller would spin forever", __FILE__, __LINE__);
  codin_shim_n_threads -= 1;
  Codin_Shim_Thread t = codin_shim_threads[codin_shim_n_threads];
  t.proc(t.arg);
}
#endif
