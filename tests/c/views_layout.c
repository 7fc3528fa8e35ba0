/* Layout of RT_View (include/rt_hip.h) as a C11 compiler sees it: tests/test_views_abi.py compares it with the ctypes mirror. */
#include <stddef.h>
#include <stdio.h>

#include "rt_hip.h"

int main(void) {
  printf("sizeof %zu\n", sizeof(RT_View));
  printf("align %zu\n", _Alignof(RT_View));
  printf("camera %zu\n", offsetof(RT_View, camera));
  printf("seed %zu\n", offsetof(RT_View, seed));
  printf("camera.focal_length %zu\n", offsetof(RT_View, camera.focal_length));
  return 0;
}
