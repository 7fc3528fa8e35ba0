/* codin/sort.h -- stand-in, written for this project (see codin.h).
 * ASSUMPTIONS about the real codin, with the reference line that uses each:
 *   S1  sort_slice_by(slice, i, j, less) sorts `slice` in place; `less` is an expression over the index names i and j
 *       that is true when element i of the slice, as it stands at that moment, goes before element j   scene.c:206-221
 *   S2  the sort is STABLE.  Unknown for the real codin: this is deviation D7 of oracle/oracle.h, shared with
 *       raytracing_c_amd/csrc/rt_scene_build.c.  THIS STAND-IN is a bottom-up merge sort; every comparison reads the
 *       slice while a merge writes to a side buffer, so `less` always sees the elements it names. */
#ifndef CODIN_SHIM_SORT_H
#define CODIN_SHIM_SORT_H
#include "codin.h"
#define sort_slice_by(s, i, j, ...) do {                                                                   \
    isize n_ = (s).len;                                                                                     \
    if (n_ < 2) break;                                                                                      \
    type_of((s).data) tmp_ = (type_of((s).data))malloc((size_t)n_ * sizeof((s).data[0]));                   \
    if (!tmp_) codin_shim_panic("out of memory", __FILE__, __LINE__);                                       \
    for (isize w_ = 1; w_ < n_; w_ *= 2) {                                                                  \
      for (isize lo_ = 0; lo_ < n_; lo_ += 2 * w_) {                                                        \
        isize mid_ = lo_ + w_ < n_ ? lo_ + w_ : n_, hi_ = lo_ + 2 * w_ < n_ ? lo_ + 2 * w_ : n_;            \
        isize a_ = lo_, b_ = mid_, k_ = lo_;                                                                \
        while (a_ < mid_ && b_ < hi_) {                                                                     \
          isize i = b_, j = a_;                       /* take the right element only when it is LESS */     \
          if (__VA_ARGS__) tmp_[k_++] = (s).data[b_++]; else tmp_[k_++] = (s).data[a_++];                   \
        }                                                                                                   \
        while (a_ < mid_) tmp_[k_++] = (s).data[a_++];                                                      \
        while (b_ < hi_)  tmp_[k_++] = (s).data[b_++];                                                      \
      }                                                                                                     \
      memcpy((s).data, tmp_, (size_t)n_ * sizeof((s).data[0]));                                             \
    }                                                                                                       \
    free(tmp_);                                                                                             \
  } while (0)
#endif
