// rt_host.cpp -- errors, configuration (read once), device slots, the seed and the material / background tokens.

#include "rt_host.h"

// ---------------------------------------------------------------------------------
// errors

static std::mutex g_err_mutex;
static char       g_err[1024] = "";

int rt_fail(const char *fmt, ...) {
  std::lock_guard<std::mutex> lock(g_err_mutex);
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  fprintf(stderr, "rt_hip: %s\n", g_err);
  return -1;
}

// rt_fail for the host units written in C (rt_scene_refit.c reaches it through a weak reference)
extern "C" __attribute__((visibility("hidden"))) void rt_error_message(char const *message) { rt_fail("%s", message); }
extern "C" char const *rt_last_error(void) { return g_err; }
extern "C" void rt_clear_error(void) {
  std::lock_guard<std::mutex> lock(g_err_mutex);
  g_err[0] = 0;
}

// ---------------------------------------------------------------------------------
// configuration: read once, never per launch (what is read: rt_host.h)

static std::mutex g_cfg_mutex;
static Config &config_locked() {
  static Config c = [] {
    Config c0;
    if (const char *e = getenv("RT_DEVICES")) {
      int v = atoi(e);
      if (v >= 1 && v <= RT_MAX_DEVICES) c0.devices = v;
    }
    if (const char *e = getenv("RT_DEVICES_REHEARSE")) c0.rehearse = atoi(e) != 0;
    return c0;
  }();
  return c;
}
Config config() {
  std::lock_guard<std::mutex> lock(g_cfg_mutex);
  return config_locked();
}

extern "C" int rt_set_devices(i32 n_devices, i32 rehearse) {
  if (n_devices < 1 || n_devices > RT_MAX_DEVICES) return rt_fail("rt_set_devices: %d outside [1, %d]", n_devices, RT_MAX_DEVICES);
  {
    std::lock_guard<std::mutex> lock(g_cfg_mutex);
    Config &c = config_locked();
    c.devices = n_devices;
    c.rehearse = rehearse != 0;
  }
  remap_device_slots();          // a slot that was mapped to another GPU under the old configuration starts over
  return 0;
}

// ---------------------------------------------------------------------------------
// per-device state

Device *const    g_devs = new Device[RT_MAX_DEVICES];   // never destroyed: no HIP call from static destruction (rt_host.h)
int              g_primary = 0;                   // physical device of slot 0
static bool      g_primary_fixed = false;         // slot 0 has been initialised (rt_init can no longer move it)
std::atomic<u32> g_seed{0x1234ABCDu};
std::mutex       g_multi_mutex;                   // counters of the last multi-device frame
RT_Counters      g_multi_counters;
bool             g_multi_counters_valid = false;

int ensure_device(Device &D) {            // D.mutex held (or single-threaded start-up)
  if (D.ready) return hipSetDevice(D.phys) == hipSuccess ? 0 : rt_fail("hipSetDevice(%d) failed", D.phys);
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    return rt_fail("no HIP device available (%s); the render path has no CPU fallback",
                   e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
  }
  if (D.slot == 0) {
    D.phys = g_primary;
    g_primary_fixed = true;
  } else {
    D.phys = config().rehearse ? g_primary : (g_primary + D.slot) % count;
  }
  if (D.phys >= count) return rt_fail("device %d requested but only %d present", D.phys, count);
  HIP_TRY(hipSetDevice(D.phys));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, D.phys));
  D.num_cus = prop.multiProcessorCount;
  if (D.slot != 0 && D.phys != g_primary) {
    // this device sends its tiles into device 0's buffer: direct xGMI copies when peer access can be enabled, staged ones otherwise
    int can = 0;
    D.peer_ok = false;
    if (hipDeviceCanAccessPeer(&can, D.phys, g_primary) == hipSuccess && can) {
      hipError_t pe = hipDeviceEnablePeerAccess(g_primary, 0);
      if (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled) D.peer_ok = true;
      if (pe != hipSuccess) (void)hipGetLastError();
    }
    // (refused: the tiles go through a pinned host buffer, render_frame_multi)
  }
  if (!D.mstream) HIP_TRY(hipStreamCreateWithFlags(&D.mstream, hipStreamNonBlocking));
  D.ready = true;
  return 0;
}

extern "C" int rt_init(int device) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (g_primary_fixed && device != g_primary) return rt_fail("rt_init: device already initialised as %d", g_primary);
  if (device < 0) return rt_fail("rt_init: device %d is invalid", device);
  g_primary = device;
  for (int i = 0; i < RT_MAX_DEVICES; i++) g_devs[i].slot = i;
  (void)config();                                 // the one read of the environment
  return ensure_device(D);
}

// GPUs a frame behind render_thread_proc / render() will be spread over on this machine right now
extern "C" i32 rt_device_count(void) {
  Config c = config();
  if (c.rehearse) return c.devices;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return 0;
  return c.devices < count ? c.devices : count;
}

extern "C" void rt_set_seed(u32 seed) { g_seed.store(seed); }
extern "C" u32  rt_get_seed(void) { return g_seed.load(); }

// ---------------------------------------------------------------------------------
// material tokens (rt_materials.h): recognised by address, not callable

extern "C" void disney_shader_proc(rawptr, Shader_Input const *, Shader_Output *output) {
  rt_fail("disney_shader_proc is a device material token and cannot be called on the host");
  if (output) output->terminate = true;
}

extern "C" void debug_shader_proc(rawptr, Shader_Input const *, Shader_Output *output) {
  rt_fail("debug_shader_proc is a device material token and cannot be called on the host");
  if (output) output->terminate = true;
}

extern "C" Color3 sample_background(Image const *, Vec3) {
  rt_fail("sample_background is a device background token and cannot be called on the host");
  Color3 c;
  c.x = c.y = c.z = 0.0f;
  return c;
}

// What rt_scene_upload compares Shader.proc / Background.proc with: this library's own exported tokens.  The diagnostic
// library can be told to recognise the PRODUCT library's tokens instead (rt_diag_set_tokens): a test process that has both
// libraries mapped builds its scenes once, with the product's addresses, and sends them through the unit-test entry points
// of the diagnostic build.
Shader_Proc     g_tok_disney = disney_shader_proc;
Shader_Proc     g_tok_debug = debug_shader_proc;
Background_Proc g_tok_background = (Background_Proc)sample_background;
