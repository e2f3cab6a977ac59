// Default library only: rb_dvis_fused's precision 5 lives in the legacy library (vis_diffuse_h3.hip).
#include "dvis_fused.h"
int rb::dvis_fused_h3(const float*, const int*, long, const float*, const float*, const float*, const float*, const float*, const float*,
                      const float*, const float*, int, int, int, int, float*, unsigned long long*, rb_stream_t) {
  return rb::fail("rb_dvis_fused", "precision 5 (first-generation split-precision kernel) is built into librobir_hip_legacy.so only (make legacy)");
}
