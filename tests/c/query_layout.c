/* Layout of RT_Ray_Hit, RT_Device_Hit, RT_Query_Counters (include/rt_hip.h) and of the reference's Hit as a C11 compiler sees them:
 * tests/test_query_abi.py compares them with each other and with the ctypes mirror. */
#include <stddef.h>
#include <stdio.h>

#include "rt_hip.h"

#define FIELD(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("sizeof.RT_Ray_Hit %zu\n", sizeof(RT_Ray_Hit));
  printf("sizeof.RT_Device_Hit %zu\n", sizeof(RT_Device_Hit));
  printf("sizeof.Hit %zu\n", sizeof(Hit));
  printf("sizeof.RT_Query_Counters %zu\n", sizeof(RT_Query_Counters));
  printf("sizeof.Ray %zu\n", sizeof(Ray));
  FIELD(RT_Ray_Hit, t); FIELD(RT_Ray_Hit, triangle); FIELD(RT_Ray_Hit, u); FIELD(RT_Ray_Hit, v);
  FIELD(RT_Device_Hit, distance); FIELD(RT_Device_Hit, normal); FIELD(RT_Device_Hit, normal_geo); FIELD(RT_Device_Hit, point);
  FIELD(RT_Device_Hit, tangent); FIELD(RT_Device_Hit, bitangent); FIELD(RT_Device_Hit, tex_coords);
  FIELD(RT_Device_Hit, triangle); FIELD(RT_Device_Hit, material); FIELD(RT_Device_Hit, pad);
  FIELD(Hit, distance); FIELD(Hit, normal); FIELD(Hit, normal_geo); FIELD(Hit, point);
  FIELD(Hit, tangent); FIELD(Hit, bitangent); FIELD(Hit, tex_coords); FIELD(Hit, shader);
  FIELD(RT_Query_Counters, rays); FIELD(RT_Query_Counters, hits); FIELD(RT_Query_Counters, node_visits);
  FIELD(RT_Query_Counters, leaf_visits);
  return 0;
}
