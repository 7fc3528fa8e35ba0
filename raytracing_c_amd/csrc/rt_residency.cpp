// rt_residency.cpp -- scene residency: the device copy of a host Scene, its upload, stamps, fingerprints and in-place edits.

#include "rt_host.h"

void free_device_scene(RT_Device_Scene *d) {      // d->dev->mutex held, d's device current
  if (!d) return;
  if (d->dev) {
    for (FrameLane &F : d->dev->lanes)        // a frame in flight renders from this copy: let it finish (its pixels are in the lane's buffer)
      if (F.busy && F.d == d) {
        if (F.stream) (void)hipStreamSynchronize(F.stream);
        F.d = nullptr;
      }
    for (LaunchState &L : d->ls)
      if (L.counters && d->dev->last_counters == L.counters) d->dev->last_counters = nullptr;
  }
  delete d;                                   // (its members own what it holds on the device, rt_mem.h)
}

template <typename T>
static int upload(DevMem<T> &dst, const std::vector<T> &src, int64_t *bytes) {
  HIP_TRY(dst.grow(src.size()));
  if (!src.empty()) HIP_TRY(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  *bytes += (int64_t)dst.bytes();
  return 0;
}

// Textures are packed to RGBA8 words ON THE GPU: the host only records which Images are used (in first-use order)
// and where each one starts in the texel pool; upload_textures() copies the raw rows and runs rt_pack_texture_kernel.
struct TexturePool {
  std::unordered_map<const Image *, int> map;
  std::vector<RT_DTexture>               descs;
  std::vector<const Image *>             sources;
  size_t                                 texels = 0;
};

static int texture_index(Image const *img, TexturePool &pool) {
  if (!img) return -1;
  auto it = pool.map.find(img);
  if (it != pool.map.end()) return it->second;
  if (img->pixel_type != PT_u8 || img->components < 3 || img->width <= 0 || img->height <= 0 || !img->pixels.data ||
      img->stride < img->width ||
      img->pixels.len < (isize)img->stride * img->height * img->components) {     // the upload reads exactly that many bytes
    return -2;
  }
  RT_DTexture t;
  t.offset = (uint32_t)pool.texels;
  t.width = (int32_t)img->width;
  t.height = (int32_t)img->height;
  t.stride = (int32_t)((img->width + 3) / 4);                                  // tiles per row (rt_device.h)
  pool.texels += (size_t)t.stride * (size_t)((img->height + 3) / 4) * 16;
  int idx = (int)pool.descs.size();
  pool.descs.push_back(t);
  pool.sources.push_back(img);
  pool.map[img] = idx;
  return idx;
}

// ... and, from the staged rows of the background (texture `bg` of the pool), rt_pack_bg_image_kernel: its float copy (rt_device.h)
static int upload_textures(const TexturePool &pool, DevMem<uint32_t> &d_texels, int bg, DevMem<float> &d_bg_image, int64_t *bytes) {
  HIP_TRY(d_texels.grow(pool.texels));
  *bytes += (int64_t)d_texels.bytes();
  const size_t bg_texels = ((size_t)pool.descs[bg].width + 1) * ((size_t)pool.descs[bg].height + 1);
  if (bg_texels * RT_BG_TEXEL_FLOATS * sizeof(float) > RT_BG_IMAGE_MAX_BYTES)
    return rt_fail("rt_scene_upload: the background (%d x %d) is too large for its float copy", pool.descs[bg].width, pool.descs[bg].height);
  if (d_bg_image.grow(bg_texels * RT_BG_TEXEL_FLOATS) != hipSuccess)
    return rt_fail("rt_scene_upload: out of device memory for the float copy of the background (%zu bytes)", bg_texels * RT_BG_TEXEL_FLOATS * sizeof(float));
  *bytes += (int64_t)d_bg_image.bytes();
  size_t max_raw = 0;
  for (const Image *img : pool.sources) {
    size_t raw = (size_t)img->stride * img->height * img->components;
    if (raw > max_raw) max_raw = raw;
  }
  if (max_raw == 0) return 0;
  DevMem<uint8_t> stage;
  HIP_TRY(stage.grow(max_raw));
  int rc = 0;
  for (size_t k = 0; k < pool.sources.size() && rc == 0; k++) {
    const Image *img = pool.sources[k];
    size_t raw = (size_t)img->stride * img->height * img->components;
    rc = (int)hipMemcpy(stage, img->pixels.data, raw, hipMemcpyHostToDevice);
    if (rc == 0) rc = rt_launch_pack_texture(stage, (int)img->width, (int)img->height, 0, (int)img->stride, (int)img->components,
                                             d_texels + pool.descs[k].offset, nullptr);
    if (rc == 0 && (int)k == bg) rc = rt_launch_pack_bg_image(stage, (int)img->width, (int)img->height, (int)img->height, 0, (int)img->stride,
                                                              (int)img->components, d_bg_image, nullptr);
    if (rc == 0) rc = (int)hipDeviceSynchronize();        // the staging buffer is reused by the next texture
  }
  if (rc != 0) return rt_fail("texture upload failed: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- stamps of a host Scene ---------------------------------------------------------------------------------
// render_thread_proc / render / lightmap_bake keep one device copy per Scene* and must notice when the host scene
// changed underneath it -- the reference reads the live Scene every frame.  Two levels:
//  * scene_stamp(), paid on EVERY frame (tens of microseconds): the dimensions and base pointers of the BVH and the
//    triangle block, the background proc and Image, every distinct material record (PBR_Shader_Data, 80 bytes) and the
//    descriptor (pointer, size, layout) of every Image a material references, IN FULL; of every block of geometry or texel
//    bytes a bounded sample (hash_sampled: blocks up to 4 KB in full, larger ones 8 runs of 512 bytes).  A rebuilt,
//    reloaded, regenerated or re-materialed scene, a changed material parameter, a swapped texture and any edit of a small
//    scene are noticed.
//  * What it can miss: an IN-PLACE edit of a few vertices or texels inside a large block (the helmet has 5 MB of geometry
//    and 50 MB of texels; hashing them, even one word in 61, cost 0.5 ms per frame in round 2).  A host that does that
//    calls rt_scene_invalidate(scene) afterwards; scene_init / scene_init_sah / scene_init_gpu /
//    scene_refit / scene_load_bytes do so themselves (scene_refit_gpu changes the copy along with the host scene).
//    scene_fingerprint() -- geometry in full, texels of large images one word in 61 -- is what rt_scene_verify() compares for
//    a host that wants the check anyway.
static inline uint64_t mix64(uint64_t h, uint64_t v) {
  h ^= v;
  h *= 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

static uint64_t hash_bytes(uint64_t seed, const void *data, size_t n, size_t stride_words = 1) {
  const unsigned char *b = (const unsigned char *)data;
  uint64_t h0 = seed ^ 0x243F6A8885A308D3ull, h1 = seed ^ 0x13198A2E03707344ull;
  uint64_t h2 = seed ^ 0xA4093822299F31D0ull, h3 = seed ^ 0x082EFA98EC4E6C89ull;
  size_t words = n / 8, i = 0;
  const size_t step = 4 * stride_words;
  for (; i + step <= words; i += step) {         // four independent chains: the multiplies pipeline
    uint64_t w0, w1, w2, w3;
    memcpy(&w0, b + 8 * i, 8);
    memcpy(&w1, b + 8 * (i + stride_words), 8);
    memcpy(&w2, b + 8 * (i + 2 * stride_words), 8);
    memcpy(&w3, b + 8 * (i + 3 * stride_words), 8);
    h0 = mix64(h0, w0); h1 = mix64(h1, w1); h2 = mix64(h2, w2); h3 = mix64(h3, w3);
  }
  uint64_t h = mix64(mix64(mix64(h0, h1), h2), h3);
  for (; i < words; i += stride_words) { uint64_t w; memcpy(&w, b + 8 * i, 8); h = mix64(h, w); }
  if (stride_words == 1)
    for (size_t k = words * 8; k < n; k++) h = mix64(h, b[k]);
  return mix64(h, (uint64_t)n);
}

static uint64_t hash_image(uint64_t h, Image const *img) {
  if (!img) return mix64(h, 0x1234u);
  int64_t desc[6] = {(int64_t)img->components, (int64_t)img->pixel_type, (int64_t)img->width, (int64_t)img->stride,
                     (int64_t)img->height, (int64_t)(uintptr_t)img->pixels.data};
  h = hash_bytes(h, desc, sizeof desc);
  if (img->pixels.data && img->pixel_type == PT_u8 && img->width > 0 && img->height > 0 && img->stride >= img->width &&
      img->components > 0) {
    size_t n = (size_t)img->stride * img->height * img->components;
    if (img->pixels.len >= (isize)n) h = hash_bytes(h, img->pixels.data, n, n > 65536 ? 61 : 1);    // small images in full
  }
  return h;
}

// The full fingerprint as a list of BLOCKS -- the dimensions, the node array, each of the nine coordinate arrays, the AoS
// records, every distinct material record, the texels of every image it references, the background image -- each with the
// host range it covers: rt_scene_touch() uses the ranges to tell the block the host says it wrote from blocks that changed
// without a word (those drop the copy instead of being absorbed into the new reference).
static void fp_image(std::vector<FpBlock> &out, Image const *img) {
  if (!img) { out.push_back({nullptr, 0, mix64(0x1234u, 0)}); return; }
  size_t n = 0;
  if (img->pixels.data && img->pixel_type == PT_u8 && img->width > 0 && img->height > 0 && img->stride >= img->width && img->components > 0) {
    n = (size_t)img->stride * img->height * img->components;
    if (img->pixels.len < (isize)n) n = 0;
  }
  out.push_back({n ? img->pixels.data : nullptr, n, hash_image(0x51ED27u, img)});
}

static const uint64_t kFpSeed = 0x452821E638D01377ull;

// hash_geometry = false (scene_refit_gpu, before its kernels run): the node array, the coordinate arrays and the AoS records get
// their ranges but no hash (h = 0); rehash_geometry_blocks() fills them in afterwards
static void scene_fingerprint_blocks(Scene const *scene, std::vector<FpBlock> &out, bool hash_geometry = true) {
  out.clear();
  const Triangles &T = scene->triangles;
  const uint64_t h0 = kFpSeed;
  auto geometry = [&](const void *p, size_t n) { out.push_back({p, n, hash_geometry ? hash_bytes(h0, p, n) : 0}); };
  int64_t dims[5] = {(int64_t)scene->bvh.depth, (int64_t)scene->bvh.last_row_offset, (int64_t)scene->bvh.nodes.len,
                     (int64_t)T.len, (int64_t)(uintptr_t)scene->background.proc};
  out.push_back({nullptr, 0, hash_bytes(h0, dims, sizeof dims)});
  if (scene->bvh.nodes.data && scene->bvh.nodes.len > 0) {
    const size_t n = (size_t)scene->bvh.nodes.len * sizeof(BVH_Node);
    geometry(scene->bvh.nodes.data, n);
  }
  if (T.len > 0 && T.x[0] && T.aos) {
    for (int k = 0; k < 3; k++) {                // the nine coordinate arrays (one block in scene_init, but not required to be)
      const float *arrs[3] = {T.x[k], T.y[k], T.z[k]};
      for (const float *a : arrs) geometry(a, (size_t)T.len * 4);
    }
    geometry(T.aos, (size_t)T.len * sizeof(Triangle_AOS));
    const void *last = nullptr;                  // distinct material records, in first-use order
    std::vector<const void *> seen;
    for (int i = 0; i < T.len; i++) {
      const Shader &sh = T.aos[i].shader;
      if (!sh.data || sh.data == last) continue;
      last = sh.data;
      bool dup = false;
      for (const void *q : seen) if (q == sh.data) { dup = true; break; }
      if (dup) continue;
      seen.push_back(sh.data);
      if (sh.proc == g_tok_disney || sh.proc == g_tok_debug) {
        const PBR_Shader_Data *m = (const PBR_Shader_Data *)sh.data;
        out.push_back({m, sizeof *m, hash_bytes(h0, m, sizeof *m)});
        fp_image(out, m->texture_albedo);
        fp_image(out, m->texture_normal);
        fp_image(out, m->texture_metal_roughness);
        fp_image(out, m->texture_emission);
      }
      if (seen.size() > 4096) break;             // pathological material counts: the pointers are in the AoS hash anyway
    }
  }
  if (scene->background.proc == g_tok_background) fp_image(out, (Image const *)scene->background.data);
}

static uint64_t fp_fold(const std::vector<FpBlock> &blocks) {
  uint64_t h = 0x452821E638D01377ull;
  for (const FpBlock &b : blocks) h = mix64(mix64(h, b.h), (uint64_t)b.bytes);
  return h;
}

uint64_t scene_fingerprint(Scene const *scene) {
  std::vector<FpBlock> blocks;
  scene_fingerprint_blocks(scene, blocks);
  return fp_fold(blocks);
}

// A bounded look at a block of bytes: blocks up to 4 KB in full, larger ones as 8 runs of 512 bytes spread evenly over the
// block (runs, not single words: a run is 8 consecutive cache lines, a strided word per line would cost a miss each).
static uint64_t hash_sampled(uint64_t h, const void *data, size_t n) {
  if (!data || n == 0) return mix64(h, 0x5EEDu);
  if (n <= 4096) return hash_bytes(h, data, n);
  const unsigned char *b = (const unsigned char *)data;
  const size_t run = 512, runs = 8, span = n - run;
  for (size_t k = 0; k < runs; k++) {
    size_t off = (span * k / (runs - 1)) & ~(size_t)7;
    h = hash_bytes(h, b + off, run);
  }
  return mix64(h, (uint64_t)n);
}

static uint64_t hash_image_desc(uint64_t h, Image const *img) {
  if (!img) return mix64(h, 0x1234u);
  int64_t desc[6] = {(int64_t)img->components, (int64_t)img->pixel_type, (int64_t)img->width, (int64_t)img->stride,
                     (int64_t)img->height, (int64_t)(uintptr_t)img->pixels.data};
  h = hash_bytes(h, desc, sizeof desc);
  if (img->pixels.data && img->pixel_type == PT_u8 && img->width > 0 && img->height > 0 && img->stride >= img->width &&
      img->components > 0) {
    size_t n = (size_t)img->stride * img->height * img->components;
    if (img->pixels.len >= (isize)n) h = hash_sampled(h, img->pixels.data, n);
  }
  return h;
}

// `mat_ptrs` / `first_tri`: the distinct material records found at upload and one triangle that uses each.  A material
// pointer is only dereferenced while that triangle still points at it (a host that replaced its materials has freed
// the old records).  Returns 0 -- never a valid stamp -- when the scene no longer matches the lists.
static uint64_t scene_stamp(Scene const *scene, const std::vector<const void *> &mat_ptrs, const std::vector<int32_t> &first_tri) {
  const Triangles &T = scene->triangles;
  int64_t head[9] = {(int64_t)scene->bvh.depth, (int64_t)scene->bvh.last_row_offset, (int64_t)scene->bvh.nodes.len, (int64_t)T.len,
                     (int64_t)(uintptr_t)scene->background.proc, (int64_t)(uintptr_t)scene->background.data,
                     (int64_t)(uintptr_t)scene->bvh.nodes.data, (int64_t)(uintptr_t)T.x[0], (int64_t)(uintptr_t)T.aos};
  uint64_t h = hash_bytes(0x452821E638D01377ull, head, sizeof head);
  if (scene->bvh.nodes.data && scene->bvh.nodes.len > 0) h = hash_sampled(h, scene->bvh.nodes.data, (size_t)scene->bvh.nodes.len * sizeof(BVH_Node));
  if (T.len > 0 && T.x[0] && T.aos) {
    for (int k = 0; k < 3; k++) {
      h = hash_sampled(h, T.x[k], (size_t)T.len * 4);
      h = hash_sampled(h, T.y[k], (size_t)T.len * 4);
      h = hash_sampled(h, T.z[k], (size_t)T.len * 4);
    }
    h = hash_sampled(h, T.aos, (size_t)T.len * sizeof(Triangle_AOS));
  }
  if (T.aos)
    for (size_t k = 0; k < mat_ptrs.size(); k++) {
      const int32_t i = first_tri[k];
      if (i < 0 || i >= T.len || T.aos[i].shader.data != mat_ptrs[k]) return 0;
      const PBR_Shader_Data *m = (const PBR_Shader_Data *)mat_ptrs[k];
      h = hash_bytes(h, m, sizeof *m);
      h = mix64(h, (uint64_t)(uintptr_t)T.aos[i].shader.proc);
      h = hash_image_desc(h, m->texture_albedo);
      h = hash_image_desc(h, m->texture_normal);
      h = hash_image_desc(h, m->texture_metal_roughness);
      h = hash_image_desc(h, m->texture_emission);
    }
  if (scene->background.proc == g_tok_background) h = hash_image_desc(h, (Image const *)scene->background.data);
  return h | 1ull;
}

static float int_bits(int32_t i) {
  float f;
  memcpy(&f, &i, 4);
  return f;
}

// one leaf tile: 9 rows x 8: vertex a, then the edges b - a and c - a (raytracer.c:115-122 computes them per visit; the fp32
// subtraction done here gives the same bits)
static void build_leaf_tile(const Triangles &T, int g, float *l) {
  for (int k = 0; k < 8; k++) {
    int i = g * 8 + k;
    volatile float e;     // keep every difference a plain IEEE fp32 subtraction
    l[0 * 8 + k] = T.x[0][i];
    e = T.x[1][i] - T.x[0][i]; l[1 * 8 + k] = e;
    e = T.x[2][i] - T.x[0][i]; l[2 * 8 + k] = e;
    l[3 * 8 + k] = T.y[0][i];
    e = T.y[1][i] - T.y[0][i]; l[4 * 8 + k] = e;
    e = T.y[2][i] - T.y[0][i]; l[5 * 8 + k] = e;
    l[6 * 8 + k] = T.z[0][i];
    e = T.z[1][i] - T.z[0][i]; l[7 * 8 + k] = e;
    e = T.z[2][i] - T.z[0][i]; l[8 * 8 + k] = e;
  }
}
static void leaf_tile_max_edge(const float *l, float &max_edge) {
  for (int row : {1, 2, 4, 5, 7, 8})
    for (int k = 0; k < 8; k++) {
      float m = fabsf(l[row * 8 + k]);
      if (!(m <= max_edge)) max_edge = m;          // a NaN sticks (every later comparison is false as well)
    }
}
// the 28-float shading record of triangle i (rt_device.h) with material id `mat`
static void build_tri_record(const Triangle_AOS &a, int mat, float *r) {
  r[0] = a.normal.x;    r[1] = a.normal.y;    r[2] = a.normal.z;    r[3] = int_bits(mat < 0 ? 0 : mat);
  r[4] = a.normal_a.x;  r[5] = a.normal_a.y;  r[6] = a.normal_a.z;  r[7] = a.tex_coords_a.x;
  r[8] = a.normal_b.x;  r[9] = a.normal_b.y;  r[10] = a.normal_b.z; r[11] = a.tex_coords_a.y;
  r[12] = a.normal_c.x; r[13] = a.normal_c.y; r[14] = a.normal_c.z; r[15] = a.tex_coords_b.x;
  r[16] = a.tangent.x;  r[17] = a.tangent.y;  r[18] = a.tangent.z;  r[19] = a.tex_coords_b.y;
  r[20] = a.bitangent.x; r[21] = a.bitangent.y; r[22] = a.bitangent.z; r[23] = a.tex_coords_c.x;
  r[24] = a.tex_coords_c.y; r[25] = 0.0f; r[26] = 0.0f; r[27] = 0.0f;
}
static void build_material_row(const PBR_Shader_Data *d, int ta, int tn, int tm, int te, int kind,
                               const std::vector<RT_DTexture> &descs, float *m) {
  const float row[20] = {d->base_color.x, d->base_color.y, d->base_color.z, d->roughness,
                         d->emission.x, d->emission.y, d->emission.z, d->metalness,
                         d->normal_map_strength, d->sheen, d->sheen_tint, d->anisotropic_strength,
                         int_bits(ta), int_bits(tn), int_bits(tm), int_bits(te),
                         int_bits(kind), 0.0f, 0.0f, 0.0f};
  memcpy(m, row, sizeof row);
  const int tex[4] = {ta, tn, tm, te};
  for (int k = 0; k < 4; k++) {
    float *q = m + 20 + 4 * k;
    if (tex[k] >= 0 && (size_t)tex[k] < descs.size()) {
      const RT_DTexture &t = descs[(size_t)tex[k]];
      q[0] = int_bits((int32_t)t.offset); q[1] = int_bits(t.width); q[2] = int_bits(t.height); q[3] = int_bits(t.stride);
    } else {
      q[0] = q[1] = q[2] = q[3] = 0.0f;
    }
  }
}

// May a shade block compute ONE set of bilinear taps for a material's four textures (SharedTaps, rt_dev.hip.h)?  Yes when, in
// every one of the n packed material rows (RT_MAT_FLOATS floats each, rt_device.h), all the textures the row names -- slot index
// >= 0 -- have the same width, height and stride in the descriptors embedded in the row.  A material with no texture or one
// agrees with itself; so does an empty table.  Conservative: one mixed material and the whole scene renders with the general form.
extern "C" int rt_materials_share_taps(const float *mats, i32 n_materials) {
  if (!mats || n_materials <= 0) return 1;
  for (i32 m = 0; m < n_materials; m++) {
    int32_t w[RT_MAT_FLOATS];
    memcpy(w, mats + (size_t)m * RT_MAT_FLOATS, sizeof w);
    int first = -1;
    for (int k = 0; k < 4; k++) {
      if (w[12 + k] < 0) continue;
      if (first < 0) { first = k; continue; }
      for (int f = 1; f < 4; f++)                                        // width, height, stride; not the offset
        if (w[20 + 4 * k + f] != w[20 + 4 * first + f]) return 0;
    }
  }
  return 1;
}

// ... of the copy's material table as it is now; and whether any material names a texture at all (a scene without one has no taps
// to share and keeps the general instance).  After every write to d->mats_host.
static void refresh_shared_taps(RT_Device_Scene *d) {
  bool any = false;
  for (size_t m = 0; m < d->mats_host.size() / RT_MAT_FLOATS && !any; m++)
    for (int k = 0; k < 4; k++) {
      int32_t t;
      memcpy(&t, &d->mats_host[m * RT_MAT_FLOATS + 12 + k], 4);
      if (t >= 0) any = true;
    }
  d->shared_taps = any && rt_materials_share_taps(d->mats_host.data(), (i32)(d->mats_host.size() / RT_MAT_FLOATS)) != 0;
}

bool node_boxes_ordered(const float *nodes, size_t n_nodes) {
  for (size_t nd = 0; nd < n_nodes; nd++)
    for (int k = 0; k < 24; k++)
      if (!(nodes[nd * 48 + k] <= nodes[nd * 48 + 24 + k])) return false;
  return true;
}

static RT_Device_Scene *upload_scene_locked(Device &D, Scene const *scene) {
  if (ensure_device(D) != 0) return nullptr;
  if (!scene) { rt_fail("rt_scene_upload: scene is NULL"); return nullptr; }
  const Triangles &T = scene->triangles;
  if (T.len <= 0 || T.len % 8 != 0 || !T.x[0] || !T.aos) {
    rt_fail("rt_scene_upload: triangle block is empty or not a multiple of 8 (len=%d)", (int)T.len);
    return nullptr;
  }
  if (scene->bvh.depth < 0 || scene->bvh.depth > RT_MAX_DEPTH) {
    rt_fail("rt_scene_upload: bvh.depth %ld outside [0, %d]", (long)scene->bvh.depth, RT_MAX_DEPTH);
    return nullptr;
  }
  if (scene->bvh.depth > 0) {
    if (scene->bvh.nodes.len < bvh_n_internal_nodes(scene->bvh.depth) || !scene->bvh.nodes.data) {
      rt_fail("rt_scene_upload: %ld nodes for depth %ld", (long)scene->bvh.nodes.len, (long)scene->bvh.depth);
      return nullptr;
    }
    if ((isize)T.len < bvh_n_leaf_nodes(scene->bvh.depth) * 8) {
      rt_fail("rt_scene_upload: %d triangle slots for depth %ld", (int)T.len, (long)scene->bvh.depth);
      return nullptr;
    }
  }
  if (scene->background.proc != g_tok_background || !scene->background.data) {
    rt_fail("rt_scene_upload: background.proc is not the exported sample_background token "
            "(host callbacks cannot run on the GPU)");
    return nullptr;
  }

  TexturePool pool;
  std::unordered_map<uint64_t, int>      mat_map;     // (data ptr, kind) -> id
  std::vector<float>                     mats;
  std::vector<const void *>              mat_ptrs;
  std::vector<int32_t>                   mat_first_tri;

  // triangles + materials
  const int n = T.len;
  std::vector<float> tris((size_t)n * 28, 0.0f);
  for (int i = 0; i < n; i++) {
    const Triangle_AOS &a = T.aos[i];
    int mat = 0;
    if (a.shader.proc == nullptr) {
      mat = -1;   // unpopulated slot: never hit (all-zero triangle)
    } else {
      int kind;
      if (a.shader.proc == g_tok_disney) kind = RT_MAT_DISNEY;
      else if (a.shader.proc == g_tok_debug) kind = RT_MAT_DEBUG;
      else {
        rt_fail("rt_scene_upload: triangle %d uses a shader proc that is not an exported device material "
                "(disney_shader_proc / debug_shader_proc)", i);
        return nullptr;
      }
      if (!a.shader.data) { rt_fail("rt_scene_upload: triangle %d has shader.data == NULL", i); return nullptr; }
      uint64_t key = (uint64_t)(uintptr_t)a.shader.data * 2u + (uint64_t)kind;
      auto it = mat_map.find(key);
      if (it != mat_map.end()) {
        mat = it->second;
      } else {
        const PBR_Shader_Data *d = (const PBR_Shader_Data *)a.shader.data;
        int ta = texture_index(d->texture_albedo, pool);
        int tn = texture_index(d->texture_normal, pool);
        int tm = texture_index(d->texture_metal_roughness, pool);
        int te = texture_index(d->texture_emission, pool);
        if (ta == -2 || tn == -2 || tm == -2 || te == -2) {
          rt_fail("rt_scene_upload: material of triangle %d references an unusable Image (need PT_u8, >= 3 components, pixels.len >= stride*height*components)", i);
          return nullptr;
        }
        mat = (int)(mats.size() / RT_MAT_FLOATS);
        float m[RT_MAT_FLOATS];
        build_material_row(d, ta, tn, tm, te, kind, pool.descs, m);
        mats.insert(mats.end(), m, m + RT_MAT_FLOATS);
        mat_map[key] = mat;
        mat_ptrs.push_back(a.shader.data);
        mat_first_tri.push_back(i);
      }
    }
    build_tri_record(a, mat, &tris[(size_t)i * 28]);
  }
  if (mats.empty()) mats.resize(RT_MAT_FLOATS, 0.0f);

  // leaf tiles (build_leaf_tile)
  const int n_groups = n / 8;
  std::vector<float> leaves((size_t)n_groups * 72);
  float max_edge = 0.0f;
  for (int g = 0; g < n_groups; g++) {
    build_leaf_tile(T, g, &leaves[(size_t)g * 72]);
    leaf_tile_max_edge(&leaves[(size_t)g * 72], max_edge);
  }

  std::vector<float> nodes;
  bool boxes_ordered = true;
  if (scene->bvh.depth > 0) {
    const float *src = (const float *)scene->bvh.nodes.data;
    nodes.assign(src, src + (size_t)scene->bvh.nodes.len * 48);
    // the LDS node blocks pick the near / far plane of a slab by the sign of the ray direction: valid for min <= max
    // (what scene_init builds; a Scene from elsewhere is checked, and traverses through the min / max form otherwise)
    boxes_ordered = node_boxes_ordered(nodes.data(), (size_t)scene->bvh.nodes.len);
  }

  int bg = texture_index((Image const *)scene->background.data, pool);
  if (bg < 0) { rt_fail("rt_scene_upload: background Image is unusable (need PT_u8, >= 3 components, pixels.len >= stride*height*components)"); return nullptr; }

  RT_Device_Scene *d = new RT_Device_Scene();
  d->dev = &D;
  if (d->ls[0].counters.grow(RT_N_COUNTERS) != hipSuccess || d->ls[0].work_head.grow(16) != hipSuccess) {
    rt_fail("rt_scene_upload: out of device memory");
    free_device_scene(d);
    return nullptr;
  }
  if (upload(d->nodes, nodes, &d->bytes) || upload(d->leaves, leaves, &d->bytes) ||
      upload(d->tris, tris, &d->bytes) || upload(d->mats, mats, &d->bytes) ||
      upload(d->textures, pool.descs, &d->bytes) || upload_textures(pool, d->texels, bg, d->bg_image, &d->bytes)) {
    free_device_scene(d);
    return nullptr;
  }
  d->depth = (int32_t)scene->bvh.depth;
  d->last_row_offset = (int32_t)scene->bvh.last_row_offset;
  d->bg_texture = bg;
  d->n_nodes = (int32_t)scene->bvh.nodes.len;
  d->n_triangles = n;
  d->max_edge = max_edge;
  d->boxes_ordered = boxes_ordered;
  d->n_materials = (int32_t)(mats.size() / RT_MAT_FLOATS);
  d->mats_host = mats;
  refresh_shared_taps(d);
  d->n_textures = (int32_t)pool.descs.size();
  d->mat_ptrs = mat_ptrs;
  d->mat_first_tri = mat_first_tri;
  d->mat_map = mat_map;
  d->tex_sources = pool.sources;
  d->tex_descs = pool.descs;
  d->stamp = scene_stamp(scene, d->mat_ptrs, d->mat_first_tri);
  return d;
}

// rt_scene_upload / release / set_camera work on the primary device (one process per GPU under torch.distributed)
extern "C" RT_Device_Scene *rt_scene_upload(Scene const *scene) {
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  RT_Device_Scene *d = upload_scene_locked(D, scene);
  if (d) D.cameras[d] = scene->camera;
  return d;
}

extern "C" void rt_scene_release(RT_Device_Scene *dscene) {
  if (!dscene) return;
  Device &D = dscene->dev ? *dscene->dev : dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  for (auto it = D.scene_cache.begin(); it != D.scene_cache.end(); ++it) {
    if (it->second == dscene) { D.scene_cache.erase(it); break; }
  }
  D.cameras.erase(dscene);
  free_device_scene(dscene);
}

static void forget_static(Scene const *scene);
extern "C" void rt_scene_invalidate(Scene const *scene) {
  forget_static(scene);             // (a Scene rebuilt or freed and allocated again at this address starts checked, like a new one)
  for (int i = 0; i < RT_MAX_DEVICES; i++) {
    Device &D = g_devs[i];
    std::lock_guard<std::mutex> lock(D.mutex);
    auto it = D.scene_cache.find(scene);
    if (it != D.scene_cache.end()) {
      DeviceGuard guard(D);
      free_device_scene(it->second);
      D.scene_cache.erase(it);
    }
  }
}

extern "C" i64 rt_scene_device_bytes(RT_Device_Scene const *dscene) { return dscene ? dscene->bytes : 0; }

// ---- kept geometry ---------------------------------------------------------------------------------------------------------
// What THE MOTION of a feature pass is measured against (include/rt_hip.h): the copy's leaf tiles as they are now, saved by ONE
// device-to-device copy before the host deforms the mesh (scene_refit_gpu rewrites d->leaves in place and keeps every triangle in
// its slot).  The snapshot is a member of the copy: whatever drops the copy -- invalidate, a re-upload, rt_scene_free, a refit that
// falls back to scene_refit, release_staging -- drops it too.

// D.mutex held, D's GPU current.
static int keep_geometry_locked(RT_Device_Scene *d, hipStream_t stream) {
  const size_t n = d->leaves.cap;                                 // 72 f32 per leaf group
  d->has_kept = false;
  HIP_TRY(d->kept_leaves.grow(n));
  if (n) HIP_TRY(hipMemcpyAsync(d->kept_leaves, d->leaves, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
  d->has_kept = true;
  return 0;
}

extern "C" int rt_device_scene_keep_geometry(RT_Device_Scene *dscene, void *stream) {
  if (!dscene) return rt_fail("rt_device_scene_keep_geometry: device scene is NULL");
  Device &D = dscene->dev ? *dscene->dev : dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  DeviceGuard guard(D);
  return keep_geometry_locked(dscene, (hipStream_t)stream);
}

extern "C" int rt_scene_keep_geometry(Scene const *scene) {
  if (!scene) return rt_fail("rt_scene_keep_geometry: scene is NULL");
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  if (ensure_device(D) != 0) return -1;
  RT_Device_Scene *d = cached_scene_locked(D, scene, nullptr, nullptr);      // (the ordinary upload when there is no copy)
  if (!d) return -1;
  return keep_geometry_locked(d, nullptr);                        // (a refit that follows waits for the device before it writes)
}

extern "C" int rt_scene_has_kept_geometry(Scene const *scene) {
  if (!scene) return 0;
  Device &D = dev0();
  std::lock_guard<std::mutex> lock(D.mutex);
  auto it = D.scene_cache.find(scene);
  return it != D.scene_cache.end() && it->second->has_kept ? 1 : 0;
}

// ---- in-place edits of a resident scene ------------------------------------------------------------------------------------
// The reference reads the live Scene every frame (raytracer.c:596-612).  Here a frame renders from the device copy, and
// three things keep the two equal:
//  1. the sampled stamp (scene_stamp) before the frame is enqueued: rebuilt / reloaded / re-materialed scenes, microseconds;
//  2. the FULL check (scene_fingerprint: every byte of the BVH, the coordinate arrays, the AoS records and the materials, the
//     texels of large images one word in 61) computed by the calling thread WHILE the GPU renders the frame; if it differs
//     from the one taken at upload the frame is thrown away, the scene uploaded again and the frame rendered again -- a
//     frame on an unchanged scene pays nothing but host time hidden behind its own kernel.  rt_scene_set_static(scene, 1)
//     turns this off for a host that promises not to edit in place (or that calls rt_scene_touch / rt_scene_invalidate);
//  3. rt_scene_touch(scene, begin, bytes): "I wrote these bytes" -- the one block they belong to is patched on every device
//     (a few texture rows, a few leaf tiles ...) instead of 80 MB being uploaded again; this is also what catches a
//     single-texel edit that the 1-in-61 sampling of (2) can miss.
static std::mutex g_static_mutex;
static std::unordered_map<const Scene *, bool> g_static_scenes;
extern "C" void rt_scene_set_static(Scene const *scene, i32 is_static) {
  std::lock_guard<std::mutex> lock(g_static_mutex);
  if (is_static) g_static_scenes[scene] = true;
  else g_static_scenes.erase(scene);
}
static void forget_static(Scene const *scene) {
  std::lock_guard<std::mutex> lock(g_static_mutex);
  g_static_scenes.erase(scene);
}
bool scene_is_static(Scene const *scene) {
  std::lock_guard<std::mutex> lock(g_static_mutex);
  return g_static_scenes.count(scene) != 0;
}

static bool range_in(const void *begin, size_t bytes, const void *block, size_t block_bytes, size_t *off) {
  const uintptr_t b = (uintptr_t)begin, k = (uintptr_t)block;
  if (!block || b < k || b + bytes > k + block_bytes) return false;
  *off = (size_t)(b - k);
  return true;
}

// Patches the device copy `d` (device D current, D.mutex held) for host bytes [begin, begin + bytes).  1 = patched,
// 0 = the range is not something that can be patched (the caller drops the copy), -1 = HIP error.
static int touch_device_scene(RT_Device_Scene *d, Scene const *scene, const void *begin, size_t bytes) {
  const Triangles &T = scene->triangles;
  const int n = (int)T.len;
  size_t off = 0;
  if ((int32_t)scene->bvh.nodes.len != d->n_nodes || n != d->n_triangles || (int32_t)scene->bvh.depth != d->depth) return 0;
  // BVH nodes: stored as they are
  if (d->n_nodes > 0 && range_in(begin, bytes, scene->bvh.nodes.data, (size_t)d->n_nodes * sizeof(BVH_Node), &off)) {
    const size_t n0 = off / sizeof(BVH_Node), n1 = (off + bytes + sizeof(BVH_Node) - 1) / sizeof(BVH_Node);
    const float *src = (const float *)scene->bvh.nodes.data;
    for (size_t nd = n0; nd < n1; nd++)
      for (int k = 0; k < 24; k++)
        if (!(src[nd * 48 + k] <= src[nd * 48 + 24 + k])) d->boxes_ordered = false;
    HIP_TRY(hipMemcpy(d->nodes + n0 * 48, src + n0 * 48, (n1 - n0) * sizeof(BVH_Node), hipMemcpyHostToDevice));
    return 1;
  }
  // coordinate arrays: the leaf tiles of the touched triangles
  for (int k = 0; k < 3; k++) {
    const float *arrs[3] = {T.x[k], T.y[k], T.z[k]};
    for (const float *arr : arrs) {
      if (!range_in(begin, bytes, arr, (size_t)n * 4, &off)) continue;
      const int g0 = (int)(off / 4) / 8, g1 = (int)((off + bytes + 3) / 4 + 7) / 8;
      std::vector<float> tiles((size_t)(g1 - g0) * 72);
      for (int g = g0; g < g1; g++) {
        build_leaf_tile(T, g, &tiles[(size_t)(g - g0) * 72]);
        leaf_tile_max_edge(&tiles[(size_t)(g - g0) * 72], d->max_edge);        // (the bound can only grow: conservative)
      }
      HIP_TRY(hipMemcpy(d->leaves + (size_t)g0 * 72, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice));
      return 1;
    }
  }
  // AoS records: the shading records of the touched triangles (their materials must be known ones)
  if (range_in(begin, bytes, T.aos, (size_t)n * sizeof(Triangle_AOS), &off)) {
    const int i0 = (int)(off / sizeof(Triangle_AOS)), i1 = (int)((off + bytes + sizeof(Triangle_AOS) - 1) / sizeof(Triangle_AOS));
    std::vector<float> recs((size_t)(i1 - i0) * 28);
    for (int i = i0; i < i1; i++) {
      const Triangle_AOS &a = T.aos[i];
      int mat = -1;
      if (a.shader.proc != nullptr) {
        int kind = a.shader.proc == g_tok_disney ? RT_MAT_DISNEY : a.shader.proc == g_tok_debug ? RT_MAT_DEBUG : -1;
        if (kind < 0 || !a.shader.data) return 0;
        auto it = d->mat_map.find((uint64_t)(uintptr_t)a.shader.data * 2u + (uint64_t)kind);
        if (it == d->mat_map.end()) return 0;                          // a material the copy does not have: upload again
        mat = it->second;
      }
      build_tri_record(a, mat, &recs[(size_t)(i - i0) * 28]);
    }
    HIP_TRY(hipMemcpy(d->tris + (size_t)i0 * 28, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
    return 1;
  }
  // a material record (its texture pointers must still be Images of the pool)
  for (size_t k = 0; k < d->mat_ptrs.size(); k++) {
    if (!range_in(begin, bytes, d->mat_ptrs[k], sizeof(PBR_Shader_Data), &off)) continue;
    const PBR_Shader_Data *m = (const PBR_Shader_Data *)d->mat_ptrs[k];
    auto tex = [&](Image const *img) -> int {
      if (!img) return -1;
      for (size_t t = 0; t < d->tex_sources.size(); t++) if (d->tex_sources[t] == img) return (int)t;
      return -2;
    };
    const int ta = tex(m->texture_albedo), tn = tex(m->texture_normal), tm = tex(m->texture_metal_roughness), te = tex(m->texture_emission);
    if (ta == -2 || tn == -2 || tm == -2 || te == -2) return 0;
    bool any = false;
    for (auto &kv : d->mat_map) {                                        // the record may serve both kinds
      if ((const void *)(uintptr_t)(kv.first / 2u) != d->mat_ptrs[k]) continue;
      float row[RT_MAT_FLOATS];
      build_material_row(m, ta, tn, tm, te, (int)(kv.first & 1u), d->tex_descs, row);
      HIP_TRY(hipMemcpy(d->mats + (size_t)kv.second * RT_MAT_FLOATS, row, sizeof row, hipMemcpyHostToDevice));
      memcpy(&d->mats_host[(size_t)kv.second * RT_MAT_FLOATS], row, sizeof row);
      any = true;
    }
    if (any) refresh_shared_taps(d);      // the material may name other textures of the pool now: the next launch picks its instance anew
    return any ? 1 : 0;
  }
  // texels of a texture (or of the background): the touched rows are packed again
  for (size_t t = 0; t < d->tex_sources.size(); t++) {
    const Image *img = d->tex_sources[t];
    const RT_DTexture &desc = d->tex_descs[t];
    if (img->width != desc.width || img->height != desc.height || img->components < 3 || img->pixel_type != PT_u8) continue;
    const size_t row_bytes = (size_t)img->stride * img->components;
    if (!range_in(begin, bytes, img->pixels.data, row_bytes * img->height, &off)) continue;
    const size_t r0 = off / row_bytes, r1 = (off + bytes + row_bytes - 1) / row_bytes;
    DevMem<uint8_t> stage;
    HIP_TRY(stage.grow((r1 - r0) * row_bytes));
    HIP_TRY(hipMemcpy(stage, (const unsigned char *)img->pixels.data + r0 * row_bytes, (r1 - r0) * row_bytes, hipMemcpyHostToDevice));
    uint32_t *tex_base = d->texels + desc.offset;
    int rc = rt_launch_pack_texture(stage, (int)img->width, (int)(r1 - r0), (int)r0, (int)img->stride,
                                    (int)img->components, tex_base, nullptr);
    // (the background's float copy: the same rows, each with its pad column, and the pad row with the last one)
    if (rc == 0 && (int)t == d->bg_texture) rc = rt_launch_pack_bg_image(stage, (int)img->width, (int)img->height, (int)(r1 - r0), (int)r0,
                                                                         (int)img->stride, (int)img->components, d->bg_image, nullptr);
    if (rc == 0) rc = (int)hipDeviceSynchronize();
    if (rc != 0) return rt_fail("rt_scene_touch: texture rows: %s", hipGetErrorString((hipError_t)rc));
    return 1;
  }
  return 0;
}

// Does the reported range [begin, begin + bytes) touch block `b`?
static bool fp_block_holds(const FpBlock &b, const void *begin, size_t bytes) {
  const uintptr_t r0 = (uintptr_t)begin, r1 = r0 + bytes, b0 = (uintptr_t)b.begin, b1 = b0 + b.bytes;
  return b.begin && r0 < b1 && b0 < r1;
}

// 0 = every resident copy was patched in place, 1 = copies were dropped (the next frame uploads), -1 = error
extern "C" int rt_scene_touch(Scene const *scene, void const *begin, size_t bytes) {
  if (!scene || !begin || bytes == 0) return rt_fail("rt_scene_touch: NULL scene or empty range");
  // The host scene as it is NOW, block by block.  A copy may be patched only if the blocks that differ from what it was made
  // from are the one(s) the caller says it wrote: anything else is an edit nobody reported, and taking the new fingerprint
  // as the reference would hide it from every later check -- such a copy is dropped instead.
  std::vector<FpBlock> now;
  scene_fingerprint_blocks(scene, now);
  int dropped = 0;
  for (int i = 0; i < RT_MAX_DEVICES; i++) {
    Device &D = g_devs[i];
    std::lock_guard<std::mutex> lock(D.mutex);
    auto it = D.scene_cache.find(scene);
    if (it == D.scene_cache.end()) continue;
    DeviceGuard guard(D);
    RT_Device_Scene *d = it->second;
    bool unreported = now.size() != d->fp_blocks.size();
    for (size_t k = 0; !unreported && k < now.size(); k++) {
      const FpBlock &a = now[k], &b = d->fp_blocks[k];
      if (a.begin != b.begin || a.bytes != b.bytes) unreported = true;
      else if (a.h != b.h && !fp_block_holds(a, begin, bytes)) unreported = true;
    }
    int rc = unreported ? 0 : touch_device_scene(d, scene, begin, (size_t)bytes);
    if (rc == 1) {
      adopt_scene_stamps(d, scene, now);
    } else {
      free_device_scene(d);
      D.scene_cache.erase(it);
      dropped += 1;
      if (rc < 0) return -1;
    }
  }
  return dropped ? 1 : 0;
}

// After the host scene and the copy `d` were changed together: d's stamp and full fingerprint become those of the host bytes
// as they are now (`now`: their blocks).  Only for blocks the caller KNOWS the copy matches: a block that changed without a word
// must drop the copy instead, or the unreported edit is hidden from every later check.
void adopt_scene_stamps(RT_Device_Scene *d, Scene const *scene, const std::vector<FpBlock> &now) {
  d->stamp = scene_stamp(scene, d->mat_ptrs, d->mat_first_tri);
  d->fp_blocks = now;
  d->full_fp = fp_fold(now);
}

// scene_refit_gpu rewrites the node array and the triangle block on both sides and nothing else.  Is a block one of those?
static bool is_geometry_block(Scene const *scene, const FpBlock &b) {
  const Triangles &T = scene->triangles;
  const uintptr_t p = (uintptr_t)b.begin, n0 = (uintptr_t)scene->bvh.nodes.data, t0 = (uintptr_t)T.x[0];
  if (!b.begin) return false;
  if (scene->bvh.nodes.len > 0 && p >= n0 && p < n0 + (size_t)scene->bvh.nodes.len * sizeof(BVH_Node)) return true;
  return T.len > 0 && p >= t0 && p < t0 + (size_t)TRIANGLES_ALLOCATION_SIZE(T.len);
}

// Before the refit kernels run: `now` = the host scene's blocks, geometry unhashed.  true when the list has the shape of the
// one `d` was made from and every block OUTSIDE the geometry -- dimensions, material records, texels, background -- still has the
// hash it had then.  An unreported edit of the geometry itself is about to be overwritten on both sides, which is harmless.
bool refit_may_keep_copy(const RT_Device_Scene *d, Scene const *scene, std::vector<FpBlock> &now) {
  scene_fingerprint_blocks(scene, now, false);
  if (now.size() != d->fp_blocks.size()) return false;
  for (size_t k = 0; k < now.size(); k++) {
    const FpBlock &a = now[k], &b = d->fp_blocks[k];
    if (a.begin != b.begin || a.bytes != b.bytes) return false;
    if (!is_geometry_block(scene, a) && a.h != b.h) return false;
  }
  return true;
}

// ... and after them, once the host Scene holds the refitted bytes: the geometry blocks are hashed, the rest keeps the hashes
// that were just compared
void rehash_geometry_blocks(Scene const *scene, std::vector<FpBlock> &now) {
  for (FpBlock &b : now)
    if (is_geometry_block(scene, b)) b.h = hash_bytes(kFpSeed, b.begin, b.bytes);
}

// Full content check of the cached device copies of `scene`: 1 = the host scene still equals what every copy was made from
// (geometry and material bytes in full, texels of large images sampled), 0 = it changed (the copies that differ are dropped
// on EVERY device, the next frame uploads again), -1 = no cached copy on the primary device.  The per-frame check is
// scene_stamp() above.
int drop_stale_copies(Scene const *scene, uint64_t now, int first_slot) {      // returns how many copies were dropped
  int dropped = 0;
  for (int i = first_slot; i < RT_MAX_DEVICES; i++) {
    Device &D = g_devs[i];
    std::lock_guard<std::mutex> lock(D.mutex);
    auto it = D.scene_cache.find(scene);
    if (it == D.scene_cache.end() || it->second->full_fp == now) continue;
    DeviceGuard guard(D);
    (void)hipDeviceSynchronize();
    free_device_scene(it->second);
    D.scene_cache.erase(it);
    dropped += 1;
  }
  return dropped;
}
extern "C" int rt_scene_verify(Scene const *scene) {
  if (!scene) return -1;
  {
    Device &D = dev0();
    std::lock_guard<std::mutex> lock(D.mutex);
    if (D.scene_cache.find(scene) == D.scene_cache.end()) return -1;
  }
  const uint64_t now = scene_fingerprint(scene);
  return drop_stale_copies(scene, now, 0) == 0 ? 1 : 0;
}

void scene_only_kparams(RT_KParams *K, RT_Device_Scene *d) {
  memset(K, 0, sizeof *K);
  K->nodes = d->nodes;
  K->leaves = d->leaves;
  K->tris = d->tris;
  K->mats = d->mats;
  K->textures = d->textures;
  K->texels = d->texels;
  K->depth = d->depth;
  K->last_row_offset = d->last_row_offset;
  K->bg_texture = d->bg_texture;
  K->n_nodes = d->n_nodes;
  K->bg_image = d->bg_image;
  K->bg_pitch = d->tex_descs[(size_t)d->bg_texture].width + 1;
}

RT_Device_Scene *cached_scene_locked(Device &D, Scene const *scene, float *stamp_ms, float *upload_ms) {
  if (!scene) { rt_fail("render: scene is NULL"); return nullptr; }
  const double t0 = now_ms();
  auto it = D.scene_cache.find(scene);
  if (it != D.scene_cache.end()) {
    RT_Device_Scene *d = it->second;
    const bool same = d->stamp == scene_stamp(scene, d->mat_ptrs, d->mat_first_tri);
    if (stamp_ms) *stamp_ms = (float)(now_ms() - t0);
    if (same) return d;
    free_device_scene(d);                        // the host scene changed since the upload
    D.scene_cache.erase(it);
  }
  const double t1 = now_ms();
  RT_Device_Scene *d = upload_scene_locked(D, scene);
  if (d) {
    D.scene_cache[scene] = d;
    scene_fingerprint_blocks(scene, d->fp_blocks);      // (every slot keeps its own: a slot can be uploaded long after slot 0)
    d->full_fp = fp_fold(d->fp_blocks);
  }
  if (upload_ms) *upload_ms = (float)(now_ms() - t1);
  return d;
}

// (in the library's export list while the callers' copies of the check left it out of line: instantiated, so that the list stays)
template size_t std::unordered_map<const Scene *, RT_Device_Scene *>::erase(const Scene *const &);

RT_Device_Scene *scene_checked_call(Device &D, Scene const *scene, hipStream_t stream, FrameTiming *T,
                                    int (*enqueue)(void *ctx, RT_Device_Scene *d), void *ctx) {
  const bool verify = scene && !scene_is_static(scene);
  for (int attempt = 0;; attempt++) {
    float stamp_ms = 0.0f, upload_ms = 0.0f;
    RT_Device_Scene *d = cached_scene_locked(D, scene, T ? &stamp_ms : nullptr, &upload_ms);
    if (!d) return nullptr;
    const double t_enq = now_ms();
    if (enqueue(ctx, d) != 0) return nullptr;
    if (T) {
      T->stamp_ms += stamp_ms;
      T->upload_ms += upload_ms;
      T->enqueue_ms = (float)(now_ms() - t_enq);
    }
    // the full content check of the host scene, on this thread, while the GPU works (see rt_scene_touch): work on an unchanged
    // scene waits for max(kernel, check) instead of kernel + check.  A copy made for this call IS the host scene.
    if (!verify || attempt > 0 || upload_ms > 0.0f) return d;
    const double t_v = now_ms();
    const bool same = scene_fingerprint(scene) == d->full_fp;
    if (T) T->verify_ms = (float)(now_ms() - t_v);
    if (same) return d;
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { rt_fail("%s failed: %s", "hipStreamSynchronize(stream)", hipGetErrorString(e)); return nullptr; }
    free_device_scene(d);
    D.scene_cache.erase(scene);
  }
}
