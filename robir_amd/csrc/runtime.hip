// Per-library process state behind common.h: the calling thread's last error, the launch check, the compute-unit count and the
// range sentinel, with the three entry points that expose them.  Every library links its own copy.
#include "../../include/robir_hip.h"
#include "common.h"

namespace rb {

static thread_local char g_err[512] = "";
char* err_buf() { return g_err; }
int device_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    cus = prop.multiProcessorCount;
  }
  return cus;
}
int persistent_grid(long rounds, int n_workgroups) {
  if (n_workgroups <= 0) n_workgroups = device_cus();
  if (n_workgroups <= 0) return -1;
  return (int)(rounds < n_workgroups ? rounds : n_workgroups);
}

// Range sentinel words (common.h): pinned host memory mapped into every device's address space, allocated once.
static unsigned* g_range_host = nullptr;
static unsigned* g_range_dev = nullptr;
static void range_init() {
  void* h = nullptr;
  if (hipHostMalloc(&h, RB_RANGE_WORDS * sizeof(unsigned), hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  memset(h, 0, RB_RANGE_WORDS * sizeof(unsigned));
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipHostFree(h);
    return;
  }
  g_range_host = static_cast<unsigned*>(h);
  g_range_dev = static_cast<unsigned*>(d);
}
unsigned* range_flags() {
  static const bool once = (range_init(), true);
  (void)once;
  return g_range_dev;
}
unsigned* range_flags_host() {
  (void)range_flags();
  return g_range_host;
}
int fail(const char* what, const char* detail) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, detail);
  return 1;
}
int check_launch(const char* kernel) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: launch failed: %s", kernel, hipGetErrorString(e));
    return 2;
  }
  return 0;
}

}  // namespace rb

using namespace rb;

extern "C" {

int rb_abi_version(void) { return RB_ABI_VERSION; }

int rb_range_check(int synchronize, rb_stream_t stream, unsigned* mask_out) {
  RB_REQUIRE(mask_out, "null pointer");
  *mask_out = 0u;
  unsigned* w = rb::range_flags_host();
  RB_REQUIRE(w, "range sentinel: pinned host memory could not be allocated / mapped");
  if (synchronize && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return rb::fail(__func__, hipGetErrorString(hipGetLastError()));
  unsigned m = 0u;
  for (int i = 0; i < RB_RANGE_WORDS; ++i) {
    volatile unsigned* p = w + i;
    if (*p) {
      m |= 1u << i;
      *p = 0u;
    }
  }
  *mask_out = m;
  return 0;
}
const char* rb_last_error(void) { return rb::err_buf(); }

}  // extern "C"
