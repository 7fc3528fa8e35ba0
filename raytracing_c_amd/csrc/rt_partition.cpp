// rt_partition.cpp -- the chunk grid and its partition across ranks, the tables' device copies, device slot remapping.

#include "rt_host.h"

extern "C" i32 rt_chunk_count(i32 width, i32 height) {
  if (width <= 0 || height <= 0) return 0;
  return ((width + RT_CHUNK_SIZE - 1) / RT_CHUNK_SIZE) * ((height + RT_CHUNK_SIZE - 1) / RT_CHUNK_SIZE);
}

// ---- image partition across ranks -------------------------------------------------------------------
// Chunk (cx, cy) of the 32x32 grid belongs to rank (cx + B * cy) mod world, a lattice whose step B is the integer
// coprime to `world` nearest to 0.618 * world (8 -> 5, 4 -> 3, 2 -> 1): every chunk column AND every chunk row is
// spread over all ranks, so a narrow expensive structure cannot land on a few of them.  Measured cost imbalance
// (slowest rank / mean, helmet and tower frames): 1.02 / 1.02 at 8 ranks against 1.07 / 1.09 for `chunk mod world`
// (which, with 60 chunk columns, gives every rank whole columns).  A rank's chunks are numbered in ascending
// global order; the tables below are the single source of that numbering for the kernels and for Python.
static int gcd_i(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

static int partition_step(int world) {
  if (world <= 1) return 0;
  double target = 0.6180339887 * world;
  int best = 1;
  double best_d = 1e30;
  for (int b = 1; b < world; b++) {
    if (gcd_i(b, world) != 1) continue;
    double dd = b > target ? b - target : target - b;
    if (dd <= best_d) { best_d = dd; best = b; }
  }
  return best;
}

extern "C" i32 rt_chunk_owner(i32 width, i32 height, i32 world, i32 chunk) {
  i32 n = rt_chunk_count(width, height);
  if (world <= 0 || chunk < 0 || chunk >= n) return -1;
  int chunks_x = (width + RT_CHUNK_SIZE - 1) / RT_CHUNK_SIZE;
  int cx = chunk % chunks_x, cy = chunk / chunks_x;
  return (i32)((cx + (int64_t)partition_step(world) * cy) % world);
}

struct Partition {
  int width = 0, height = 0, world = 0;
  int n_chunks = 0, max_local = 0;
  std::vector<std::vector<int32_t>> lists;      // [rank] -> ascending global chunk indices
  std::vector<int32_t>              owner_slot; // [chunk] -> rank * max_local + slot
};
static std::vector<Partition *> g_partitions;
static std::mutex               g_partition_mutex;   // the host tables and every Device::parts

// The device copies of an evicted partition are not freed at once: device_chunk_list() / device_owner_table() hand out the
// pointers and release g_partition_mutex before the kernel that reads them is enqueued (under the device's own mutex), and
// another thread's 17th distinct (width, height, world) may evict in between.  They are RETIRED and freed by the eviction
// after the next one -- every frame synchronises before it returns, so whatever read them has long finished by then.
namespace { struct RetiredTables { int phys; DevPartition tables; }; }
// [0]: retired by the latest eviction, [1]: by the one before; never destroyed (no HIP call from static destruction, rt_host.h)
static std::vector<RetiredTables> *const g_retired = new std::vector<RetiredTables>[2];
static void retire(Device &D, DevPartition &&dp) { g_retired[0].push_back({D.phys, std::move(dp)}); }      // g_partition_mutex held
static void drop_device_partitions(const Partition *q) {        // g_partition_mutex held
  for (RetiredTables &rb : g_retired[1]) {                      // freed with their device current
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != rb.phys) (void)hipSetDevice(rb.phys);
    rb.tables = DevPartition();
    if (prev >= 0 && prev != rb.phys) (void)hipSetDevice(prev);
  }
  g_retired[1].swap(g_retired[0]);
  g_retired[0].clear();
  for (int i = 0; i < RT_MAX_DEVICES; i++) {
    Device &D = g_devs[i];
    for (size_t k = 0; k < D.parts.size(); k++) {
      if (D.parts[k].host != q) continue;
      retire(D, std::move(D.parts[k]));
      D.parts.erase(D.parts.begin() + (long)k);
      break;
    }
  }
}

// Gives back the staging a device keeps between host-level calls: one line per staging struct of Device.  D.mutex held, D's GPU
// current, device idle.
void release_staging(Device &D) {
  release_query_state(D);                       // (also forgets that D was the last device to answer a query)
  D.features = FeatureState();
  release_probe_state(D);                       // (also forgets that D was the last device to trace probes)
  release_lightmap_state(D);                    // (likewise for lightmaps)
  D.guided = GuidedState();
  D.refit = RefitState();
  D.upsample = UpsampleState();
  D.adaptive = AdaptiveState();
  release_temporal_state(D);                    // (also empties every live RT_History; the list of them stays)
}

// After rt_set_devices(): slot r >= 1 belongs to GPU (primary + r) mod count, or to the primary GPU when rehearsing.  A slot
// that was initialised under the other mapping gives back what it holds on the old GPU -- scene copies, frame buffers,
// events, partition tables -- and is initialised again by its next frame.
void remap_device_slots() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return;
  // A multi-device frame holds slot 0's mutex from start to end and keeps using the other slots' events, pinned buffers and
  // streams after their workers have released THEIR mutexes (gather, counter sums): tearing a slot down needs slot 0's mutex
  // first.  Lock order everywhere: slot 0 -> slot r -> g_partition_mutex.
  std::lock_guard<std::mutex> frame_lock(dev0().mutex);
  const Config c = config();
  for (int r = 1; r < RT_MAX_DEVICES; r++) {
    Device &D = g_devs[r];
    std::lock_guard<std::mutex> lock(D.mutex);
    if (!D.ready) continue;
    const int want = c.rehearse ? g_primary : (g_primary + r) % count;
    if (want == D.phys) continue;
    {
      DeviceGuard guard(D);
      (void)hipDeviceSynchronize();
      for (auto &kv : D.scene_cache) free_device_scene(kv.second);
      D.scene_cache.clear();
      D.cameras.clear();
      D.ws = Workspace();
      if (D.mstream) { (void)hipStreamDestroy(D.mstream); D.mstream = nullptr; }
      D.last_counters = nullptr;
      release_staging(D);
    }
    {
      std::lock_guard<std::mutex> pl(g_partition_mutex);
      for (DevPartition &dp : D.parts) retire(D, std::move(dp));
      D.parts.clear();
    }
    D.ready = false;
  }
}

static Partition *get_partition(int width, int height, int world) {      // g_partition_mutex held
  for (Partition *q : g_partitions)
    if (q->width == width && q->height == height && q->world == world) return q;
  if (g_partitions.size() >= 16) {              // bounded cache: forget the oldest
    Partition *old = g_partitions.front();
    drop_device_partitions(old);
    delete old;
    g_partitions.erase(g_partitions.begin());
  }
  Partition *q = new Partition();
  q->width = width; q->height = height; q->world = world;
  q->n_chunks = rt_chunk_count(width, height);
  q->lists.resize((size_t)world);
  for (int c = 0; c < q->n_chunks; c++) q->lists[(size_t)rt_chunk_owner(width, height, world, c)].push_back(c);
  for (auto &l : q->lists) if ((int)l.size() > q->max_local) q->max_local = (int)l.size();
  q->owner_slot.resize((size_t)q->n_chunks);
  for (int r = 0; r < world; r++)
    for (size_t k = 0; k < q->lists[(size_t)r].size(); k++) q->owner_slot[(size_t)q->lists[(size_t)r][k]] = r * q->max_local + (int)k;
  g_partitions.push_back(q);
  return q;
}

bool partition_args_ok(i32 width, i32 height, i32 world) {
  return width > 0 && height > 0 && world > 0 && world <= (1 << 20) && (int64_t)width * height <= ((int64_t)1 << 28);
}

extern "C" i32 rt_local_chunk_count(i32 width, i32 height, i32 rank, i32 world) {
  if (!partition_args_ok(width, height, world) || rank < 0 || rank >= world) return 0;
  std::lock_guard<std::mutex> lock(g_partition_mutex);
  return (i32)get_partition(width, height, world)->lists[(size_t)rank].size();
}

extern "C" i32 rt_max_local_chunk_count(i32 width, i32 height, i32 world) {
  if (!partition_args_ok(width, height, world)) return 0;
  std::lock_guard<std::mutex> lock(g_partition_mutex);
  return (i32)get_partition(width, height, world)->max_local;
}

extern "C" i32 rt_local_chunk_list(i32 width, i32 height, i32 rank, i32 world, i32 *out, i32 capacity) {
  if (!partition_args_ok(width, height, world) || rank < 0 || rank >= world) return 0;
  std::lock_guard<std::mutex> lock(g_partition_mutex);
  const std::vector<int32_t> &l = get_partition(width, height, world)->lists[(size_t)rank];
  for (size_t k = 0; k < l.size() && out && (i32)k < capacity; k++) out[k] = l[k];
  return (i32)l.size();
}

static DevPartition &device_partition(Device &D, const Partition *q) {     // g_partition_mutex held
  for (DevPartition &dp : D.parts)
    if (dp.host == q) return dp;
  D.parts.emplace_back();
  D.parts.back().host = q;
  D.parts.back().d_lists.resize((size_t)q->world);
  return D.parts.back();
}

// device copy of a rank's chunk list / of the owner table on D (D's GPU is the current device)
int device_chunk_list(Device &D, int width, int height, int rank, int world, const int32_t **d_list, int *n_local) {
  std::lock_guard<std::mutex> lock(g_partition_mutex);
  Partition *q = get_partition(width, height, world);
  DevPartition &dp = device_partition(D, q);
  const std::vector<int32_t> &l = q->lists[(size_t)rank];
  DevMem<int32_t> &list = dp.d_lists[(size_t)rank];
  if (!list) {
    DevMem<int32_t> fresh;                       // (kept only once it is filled)
    HIP_TRY(fresh.grow(l.size()));
    if (!l.empty()) HIP_TRY(hipMemcpy(fresh, l.data(), l.size() * 4, hipMemcpyHostToDevice));
    list = std::move(fresh);
  }
  *d_list = list;
  *n_local = (int)l.size();
  return 0;
}

int device_owner_table(Device &D, int width, int height, int world, const int32_t **d_table, int *n_chunks) {
  std::lock_guard<std::mutex> lock(g_partition_mutex);
  Partition *q = get_partition(width, height, world);
  DevPartition &dp = device_partition(D, q);
  if (!dp.d_owner_slot) {
    DevMem<int32_t> fresh;
    HIP_TRY(fresh.grow(q->owner_slot.size()));
    HIP_TRY(hipMemcpy(fresh, q->owner_slot.data(), q->owner_slot.size() * 4, hipMemcpyHostToDevice));
    dp.d_owner_slot = std::move(fresh);
  }
  *d_table = dp.d_owner_slot;
  *n_chunks = q->n_chunks;
  return 0;
}
