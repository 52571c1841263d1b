// rp_host.cpp -- librp_host.so: host-side loaders and helpers (include/rp_host.h).
#include "../../include/rp_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "rp_accum.h"
#include "rp_bvh.h"
#include "rp_denoise.h"
#include "rp_variance.h"
#include "rp_draw.h"
#include "rp_isect.h"
#include "rp_kernel.h"
#include "rp_ray.h"
#include "rp_reproject.h"
#include "rp_schedule.h"
#include "rp_units.h"

namespace {

thread_local std::string g_err;

int fail(const std::string& m) {
  g_err = m;
  return RP_EINVAL;
}

// ---- OBJ (mesh.rs:39-183) ------------------------------------------------------------------------

struct Cursor {
  const char* p;
};

bool space1(Cursor& c) {  // nom space1: one or more ' ' / '\t'
  if (*c.p != ' ' && *c.p != '\t') return false;
  while (*c.p == ' ' || *c.p == '\t') c.p++;
  return true;
}

// nom 7 number::complete::double: sign, digits, '.', digits, exponent; or inf/infinity/nan.
bool number(Cursor& c, double& out) {
  const char* s = c.p;
  const char* q = s;
  if (*q == '+' || *q == '-') q++;
  for (const char* w : {"infinity", "inf", "nan"}) {
    size_t n = std::strlen(w);
    if (strncasecmp(q, w, n) == 0) {
      std::string tok(s, (size_t)(q - s) + n);
      out = std::strtod(tok.c_str(), nullptr);
      c.p = q + n;
      return true;
    }
  }
  int digits = 0;
  while (*q >= '0' && *q <= '9') q++, digits++;
  if (*q == '.') {
    q++;
    while (*q >= '0' && *q <= '9') q++, digits++;
  }
  if (!digits) return false;
  if (*q == 'e' || *q == 'E') {
    const char* e = q + 1;
    if (*e == '+' || *e == '-') e++;
    if (*e >= '0' && *e <= '9') {
      while (*e >= '0' && *e <= '9') e++;
      q = e;
    }
  }
  std::string tok(s, (size_t)(q - s));
  out = std::strtod(tok.c_str(), nullptr);  // correctly rounded, as Rust's str::parse::<f64>
  c.p = q;
  return true;
}

struct ObjIndex {
  uint32_t p;
  int64_t n, t;  // -1 = None
  bool operator==(const ObjIndex& o) const { return p == o.p && n == o.n && t == o.t; }
};
struct ObjIndexHash {
  size_t operator()(const ObjIndex& k) const {
    uint64_t h = (uint64_t)k.p * 0x9E3779B97F4A7C15ull;
    h ^= (uint64_t)(k.n + 1) * 0xBF58476D1CE4E5B9ull + (h << 6) + (h >> 2);
    h ^= (uint64_t)(k.t + 1) * 0x94D049BB133111EBull + (h << 6) + (h >> 2);
    return (size_t)h;
  }
};

// parse_index (mesh.rs:59-71): separated_list1(tag("/"), opt(integer)).
// Returns 1 ok, 0 "position index not provided" (the face parser stops), -1 fatal (index 0 underflow).
int parse_index(Cursor& c, ObjIndex& out) {
  std::vector<int64_t> vals;
  const char* q = c.p;
  for (;;) {
    uint64_t v = 0;
    int nd = 0;
    bool ovf = false;
    while (*q >= '0' && *q <= '9') {
      v = v * 10 + (uint64_t)(*q - '0');
      if (v > 0xffffffffull) ovf = true;
      q++, nd++;
    }
    vals.push_back(nd && !ovf ? (int64_t)v : -1);
    if (*q == '/') {
      q++;
      continue;
    }
    break;
  }
  if (vals[0] < 0) return 0;
  auto conv = [](int64_t v, int64_t& o) -> bool {
    if (v < 0) { o = -1; return true; }
    if (v == 0) return false;  // `x - 1` on u32 0: the reference panics
    o = v - 1;
    return true;
  };
  int64_t p;
  if (!conv(vals[0], p)) return -1;
  out.p = (uint32_t)p;
  out.t = -1;
  out.n = -1;
  if (vals.size() > 1 && !conv(vals[1], out.t)) return -1;
  if (vals.size() > 2 && !conv(vals[2], out.n)) return -1;
  c.p = q;
  return 1;
}

// ---- sky panorama --------------------------------------------------------------------------------

double hash01(int64_t x, int64_t y, int64_t seed) {
  // randomness.rs noise::integer restated, mapped to [0, 1)
  uint64_t h = 0x369E6D3B899E43CFull * (uint64_t)x + 0x53F89E7FFDA3B07Dull * (uint64_t)y +
               0x577C2C6E4019D645ull * (uint64_t)seed;
  h = (uint64_t)((int64_t)h >> 13) ^ h;
  h = h * (h * h * 60493ull + 19990303ull) + 1376312589ull;
  return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

double smooth(double t) { return t * t * (3.0 - 2.0 * t); }

// Value noise on a lattice that wraps horizontally every `period` cells (seamless at u = 0 / 1).
double value_noise(double x, double y, int64_t period, int64_t seed) {
  double fx = std::floor(x), fy = std::floor(y);
  int64_t ix = (int64_t)fx, iy = (int64_t)fy;
  double tx = smooth(x - fx), ty = smooth(y - fy);
  auto w = [&](int64_t a) { return ((a % period) + period) % period; };
  double a = hash01(w(ix), iy, seed), b = hash01(w(ix + 1), iy, seed);
  double c = hash01(w(ix), iy + 1, seed), d = hash01(w(ix + 1), iy + 1, seed);
  double ab = a + (b - a) * tx, cd = c + (d - c) * tx;
  return ab + (cd - ab) * ty;
}

uint8_t quant(double x) {
  if (!(x > 0.0)) return 0;
  if (x >= 1.0) return 255;
  return (uint8_t)(x * 255.0 + 0.5);
}

// The slab test's terms over one node, per axis: the plane slope and the near and far addends -- the ray's own
// {inv, nb, fb} (rp_ray.h) for f32 planes, a frame's {A, Bn, Bf} (rp_isect.h frame_axis) for 8-bit codes.
struct Slabs {
  float A[3], Bn[3], Bf[3];
};
template <class Node>
Slabs frame_slabs(const Node& nd, const Slabs& ray) {
  Slabs f;
  for (int k = 0; k < 3; k++) {
    const rpi::FrameAxis a = rpi::frame_axis(nd.o[k], nd.s[k], ray.A[k], ray.Bn[k], ray.Bf[k]);
    f.A[k] = a.A;
    f.Bn[k] = a.Bn;
    f.Bf[k] = a.Bf;
  }
  return f;
}
// The children of a node (Node4: f32 planes; Node4Q, Node8Q: codes) that pass the slab test, as a bit mask, and every
// child's tnear.  Both planes with each addend and min / max where the kernel picks the near and the far plane by the
// slope's sign: the same pair of values.
template <class Node>
uint32_t children_hit(const Node& nd, const Slabs& s, float tmin32, float best32, float* tn) {
  const decltype(&nd.lo_x[0]) lo[3] = {nd.lo_x, nd.lo_y, nd.lo_z}, hi[3] = {nd.hi_x, nd.hi_y, nd.hi_z};
  uint32_t hits = 0;
  for (int c = 0; c < (int)(sizeof nd.lo_x / sizeof nd.lo_x[0]); c++) {
    float tnear = tmin32, tfar = best32;
    for (int k = 0; k < 3; k++) {
      const float l = (float)lo[k][c], h = (float)hi[k][c];
      tnear = fmaxf(tnear, fminf(rpi::plane_t(l, s.A[k], s.Bn[k]), rpi::plane_t(h, s.A[k], s.Bn[k])));
      tfar = fminf(tfar, fmaxf(rpi::plane_t(l, s.A[k], s.Bf[k]), rpi::plane_t(h, s.A[k], s.Bf[k])));
    }
    tn[c] = tnear;
    if (rpi::slab_pass(tnear, tfar)) hits |= 1u << c;
  }
  return hits;
}

// One exact test of a primitive with geometry g (rpl::Prim::g); accepted: take(t, u, v) (a sphere: u = v = 0).
template <class Take>
void prim_test(uint32_t kind, const double* g, rpi::V3 o, rpi::V3 d, double tmin, double best, Take take) {
  const rpi::V3 g0 = {g[0], g[1], g[2]};
  if (kind == rpl::PRIM_TRIANGLE) rpi::tri_test(g0, {g[3], g[4], g[5]}, {g[6], g[7], g[8]}, o, d, tmin, best, take);
  else rpi::sphere_test(g0, g[3], o, d, tmin, best, [&](double t) { take(t, 0.0, 0.0); });
}

// ---- the unit fetch on the CPU (rp_units.h; rph_unit_walk) ------------------------------------------

// One simulated launch: its arguments, its queue words, and what the environment saw.
struct UnitWalk {
  rpk::KArgs a{};
  uint32_t words[rpk::QUEUE_WORDS] = {};
  uint32_t entries[rpk::QUEUE_WORDS] = {};  // per word: fetches that got an entry (the vote's lane was not drained)
  bool probe = false;
  uint32_t block = 0;       // the fetching block
  uint32_t last_word = 0, last_q = 0;  // the fetch the next vote is about
  // the forced vote (rp_host.h rph_unit_walk any_every): queue_entries[w] = the entries of word w's queue
  uint32_t any_every = 0;
  const uint32_t* queue_entries = nullptr;
  uint64_t votes = 0, forced = 0;
  const char* err = nullptr;
};

// What fetch_pixel needs from the place it runs in (rp_device.h DevEnv is the GPU's): a wave of one lane.
struct HostEnv {
  static thread_local UnitWalk* w;
  static const rpk::KArgs* args() { return &w->a; }
  // a fetch may touch the word of a queue below queue_groups, a probe only the one word it was given
  static uint32_t fetch_add(unsigned int* p) {
    const ptrdiff_t i = p - w->words;
    const uint32_t G = std::max(w->a.P.queue_groups, 1u);
    const bool ok = i >= 0 && i < (ptrdiff_t)rpk::QUEUE_WORDS &&
                    (w->probe ? i == rpk::QUEUE_PROBE : i % rpk::QUEUE_STRIDE == 0 && i / rpk::QUEUE_STRIDE < (ptrdiff_t)G);
    if (!ok) {
      w->err = "unit walk: a fetch touched a queue word outside the launch's queues";
      w->last_word = 0;
      return w->last_q = 0xffffffffu;  // drained, whatever the queue: the walk ends without touching memory
    }
    w->last_word = (uint32_t)i;
    return w->last_q = w->words[i]++;
  }
  static bool any(bool drained) {
    w->votes++;
    if (drained) return true;
    w->entries[w->last_word]++;
    if (w->any_every && w->votes % w->any_every == 0 && w->last_q + 1 == w->queue_entries[w->last_word]) {
      w->forced++;
      return true;
    }
    return false;
  }
  static uint32_t uniform(uint32_t x) { return x; }
  static uint32_t block() { return w->block; }
  static uint32_t numerator(uint32_t n) {
    if (n >= (1u << 31)) w->err = "unit walk: a launch-constant division's numerator is 2^31 or more";
    return n;
  }
};
thread_local UnitWalk* HostEnv::w = nullptr;

// n_blocks one-lane blocks fetch in rounds until each has retired on a failed fetch; units (may be NULL): the fetched
// units, RPH_UNIT_WORDS each, up to cap.  Returns the units fetched.
template <bool PROBE>
uint64_t walk_units(UnitWalk& W, uint32_t n_blocks, uint32_t* units, uint64_t cap) {
  HostEnv::w = &W;
  std::vector<uint8_t> retired(n_blocks, 0);
  uint64_t n = 0;
  for (uint32_t live = n_blocks; live && !W.err;) {
    for (uint32_t b = 0; b < n_blocks && !W.err; b++) {
      if (retired[b]) continue;
      W.block = b;
      uint32_t slot = 0, pi = 0, pj = 0, batch = 0;
      if (!rpk::fetch_pixel<PROBE, HostEnv>(slot, pi, pj, batch)) {
        retired[b] = 1;
        live--;
        continue;
      }
      if (PROBE) W.entries[rpk::QUEUE_PROBE]++;  // (the probe's fetch takes no vote)
      if (units && n < cap) {
        const rpk::KArgs* A = &W.a;
        const uint32_t u[RPH_UNIT_WORDS] = {slot, pi, pj, batch, b, W.last_word / rpk::QUEUE_STRIDE,
                                           rpk::unit_frame(A, batch), rpk::unit_spp(A, batch)};
        std::memcpy(units + RPH_UNIT_WORDS * n, u, sizeof u);
      }
      n++;
    }
  }
  HostEnv::w = nullptr;
  return n;
}

}  // namespace

extern "C" {

const char* rph_last_error(void) { return g_err.c_str(); }

void rph_free(void* p) { std::free(p); }

void rph_mesh_free(rph_mesh* m) {
  if (!m) return;
  std::free(m->positions);
  std::free(m->normals);
  std::free(m->uvs);
  std::free(m->indices);
  std::memset(m, 0, sizeof *m);
}

int rph_obj_load(const char* path, rph_mesh* out) {
  if (!out || !path) return fail("NULL argument");
  std::memset(out, 0, sizeof *out);
  std::ifstream f(path, std::ios::binary);
  if (!f) return fail(std::string("cannot open ") + path);
  std::vector<double> P, N, T;
  std::vector<ObjIndex> verts;
  std::vector<std::pair<uint32_t, uint32_t>> faces;  // first vertex, count
  std::string line;
  while (std::getline(f, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
    Cursor c{line.c_str()};
    double v[3];
    // alt((v, vn, vt, f)) (mesh.rs:88-95); a line none of them parses is skipped (mesh.rs:117-120)
    if (c.p[0] == 'v' && (c.p[1] == ' ' || c.p[1] == '\t')) {
      c.p += 1;
      if (space1(c) && number(c, v[0]) && space1(c) && number(c, v[1]) && space1(c) && number(c, v[2]))
        P.insert(P.end(), v, v + 3);
    } else if (c.p[0] == 'v' && c.p[1] == 'n') {
      c.p += 2;
      if (space1(c) && number(c, v[0]) && space1(c) && number(c, v[1]) && space1(c) && number(c, v[2]))
        N.insert(N.end(), v, v + 3);
    } else if (c.p[0] == 'v' && c.p[1] == 't') {
      c.p += 2;
      if (space1(c) && number(c, v[0]) && space1(c) && number(c, v[1])) T.insert(T.end(), v, v + 2);
    } else if (c.p[0] == 'f') {
      c.p += 1;
      if (!space1(c)) continue;
      ObjIndex idx;
      int r = parse_index(c, idx);
      if (r < 0) return fail("face index 0 (1-based indices underflow)");
      if (r == 0) continue;
      uint32_t first = (uint32_t)verts.size(), cnt = 0;
      for (;;) {
        verts.push_back(idx);
        cnt++;
        Cursor save = c;
        if (!space1(c)) break;
        r = parse_index(c, idx);
        if (r < 0) return fail("face index 0 (1-based indices underflow)");
        if (r == 0) {
          c = save;
          break;
        }
      }
      faces.emplace_back(first, cnt);
    }
  }
  // mesh.rs:151-166: unique (p, n, t) tuples in first-use order
  std::unordered_map<ObjIndex, uint32_t, ObjIndexHash> uniq;
  uniq.reserve(verts.size() * 2 + 1);
  std::vector<uint32_t> remap(verts.size());
  std::vector<double> pos, nrm, uv;
  for (size_t k = 0; k < verts.size(); k++) {
    const ObjIndex& key = verts[k];
    auto it = uniq.find(key);
    if (it == uniq.end()) {
      if ((size_t)key.p * 3 >= P.size() || (key.n >= 0 && (size_t)key.n * 3 >= N.size()) ||
          (key.t >= 0 && (size_t)key.t * 2 >= T.size()))
        return fail("face references a missing v/vn/vt (index out of bounds)");
      uint32_t id = (uint32_t)(pos.size() / 3);
      uniq.emplace(key, id);
      pos.insert(pos.end(), &P[3 * (size_t)key.p], &P[3 * (size_t)key.p] + 3);
      if (key.n >= 0) nrm.insert(nrm.end(), &N[3 * (size_t)key.n], &N[3 * (size_t)key.n] + 3);
      else nrm.insert(nrm.end(), {0.0, 0.0, 0.0});
      if (key.t >= 0) uv.insert(uv.end(), &T[2 * (size_t)key.t], &T[2 * (size_t)key.t] + 2);
      else uv.insert(uv.end(), {0.0, 0.0});
      remap[k] = id;
    } else {
      remap[k] = it->second;
    }
  }
  std::vector<uint32_t> indices;
  indices.reserve(faces.size() * 3);
  for (auto& fc : faces) {
    if (fc.second != 3) return fail("Non-triangular face are not supported");  // mesh.rs:170-172
    for (uint32_t q = 0; q < 3; q++) indices.push_back(remap[fc.first + q]);
  }
  uint32_t nv = (uint32_t)(pos.size() / 3);
  out->n_vertices = nv;
  out->n_indices = (uint32_t)indices.size();
  out->positions = (double*)std::malloc(sizeof(double) * (pos.size() + 1));
  out->normals = (double*)std::malloc(sizeof(double) * (nrm.size() + 1));
  out->uvs = (double*)std::malloc(sizeof(double) * (uv.size() + 1));
  out->indices = (uint32_t*)std::malloc(sizeof(uint32_t) * (indices.size() + 1));
  if (!out->positions || !out->normals || !out->uvs || !out->indices) {
    rph_mesh_free(out);
    return fail("out of memory");
  }
  if (!pos.empty()) std::memcpy(out->positions, pos.data(), sizeof(double) * pos.size());
  if (!nrm.empty()) std::memcpy(out->normals, nrm.data(), sizeof(double) * nrm.size());
  if (!uv.empty()) std::memcpy(out->uvs, uv.data(), sizeof(double) * uv.size());
  if (!indices.empty()) std::memcpy(out->indices, indices.data(), sizeof(uint32_t) * indices.size());
  return RP_OK;
}

int rph_tga_load(const char* path, uint32_t* width, uint32_t* height, uint8_t** rgba) {
  if (!path || !width || !height || !rgba) return fail("NULL argument");
  std::ifstream f(path, std::ios::binary);
  if (!f) return fail(std::string("cannot open ") + path);
  uint8_t hd[18];
  if (!f.read(reinterpret_cast<char*>(hd), 18)) return fail("truncated TGA header");
  const uint32_t w = hd[12] | (hd[13] << 8), h = hd[14] | (hd[15] << 8);
  const uint8_t bpp = hd[16], desc = hd[17];
  // image.rs:81-88
  if (hd[0] != 0 || hd[1] != 0 || hd[2] != 2 || (bpp != 24 && bpp != 32))
    return fail("This tga header is not supported");
  const size_t bytes = (size_t)w * h * (bpp / 8);
  std::vector<uint8_t> raw(bytes);
  if (bytes && !f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)bytes)) return fail("truncated TGA data");
  uint8_t* img = (uint8_t*)std::malloc((size_t)w * h * 4 + 1);
  if (!img) return fail("out of memory");
  const size_t step = bpp / 8;
  for (uint32_t y0 = 0; y0 < h; y0++) {
    const uint32_t y = (desc & (1 << 5)) ? h - 1 - y0 : y0;  // image.rs:95-99 (top-left origin -> flip)
    for (uint32_t x = 0; x < w; x++) {
      const uint8_t* s = &raw[((size_t)y0 * w + x) * step];
      uint8_t* o = img + 4 * ((size_t)x + (size_t)y * w);
      o[0] = s[2];
      o[1] = s[1];
      o[2] = s[0];
      o[3] = bpp == 32 ? s[3] : 0xff;
    }
  }
  *width = w;
  *height = h;
  *rgba = img;
  return RP_OK;
}

int rph_tga_save(const char* path, uint32_t width, uint32_t height, const uint8_t* rgba) {
  if (!path || (!rgba && (uint64_t)width * height != 0)) return fail("NULL argument");
  if (width > 65535 || height > 65535) return fail("image too large for a TGA header (u16 try_into)");
  std::ofstream f(path, std::ios::binary);
  if (!f) return fail(std::string("cannot create ") + path);
  uint8_t hd[18] = {0};
  hd[2] = 2;
  hd[16] = 32;
  hd[12] = (uint8_t)width;
  hd[13] = (uint8_t)(width >> 8);
  hd[14] = (uint8_t)height;
  hd[15] = (uint8_t)(height >> 8);
  f.write(reinterpret_cast<const char*>(hd), 18);
  std::vector<uint8_t> row((size_t)width * 4);
  for (uint32_t y = 0; y < height; y++) {
    for (uint32_t x = 0; x < width; x++) {
      const uint8_t* p = rgba + 4 * ((size_t)x + (size_t)y * width);
      row[4 * x] = p[2];
      row[4 * x + 1] = p[1];
      row[4 * x + 2] = p[0];
      row[4 * x + 3] = p[3];
    }
    f.write(reinterpret_cast<const char*>(row.data()), (std::streamsize)row.size());
  }
  return f ? RP_OK : fail("write failed");
}

void rph_to_srgb_u8(const double* rgb, uint64_t n, uint8_t* rgba) {
  for (uint64_t i = 0; i < n; i++) {
    for (int c = 0; c < 3; c++) {
      double x = rgb[3 * i + c];
      if (x < 0.0) x = 0.0;  // f64::clamp keeps NaN; powf(NaN) = NaN; `as u8` maps NaN to 0
      if (x > 1.0) x = 1.0;
      double y = 255.0 * std::pow(x, 1.0 / 2.2);
      rgba[4 * i + c] = !(y > 0.0) ? 0 : (y >= 255.0 ? 255 : (uint8_t)y);
    }
    rgba[4 * i + 3] = 0xff;
  }
}

void rph_lookat(const double position[3], const double target[3], const double up[3], double orientation[9]) {
  double z[3] = {position[0] - target[0], position[1] - target[1], position[2] - target[2]};
  const double n = std::sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
  for (double& c : z) c = c / n;
  const double x[3] = {up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]};
  const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
  for (int k = 0; k < 3; k++) {
    orientation[k] = x[k];
    orientation[3 + k] = y[k];
    orientation[6 + k] = z[k];
  }
}

int rph_sky_panorama(uint32_t width, uint32_t height, uint8_t* rgba) {
  if (!rgba || width == 0 || height == 0) return fail("bad arguments");
  const double sun_u = 0.30, sun_v = 0.78;  // azimuth / elevation of the sun in texture space
  for (uint32_t j = 0; j < height; j++) {
    const double v = ((double)j + 0.5) / (double)height;  // 0 = nadir, 1 = zenith
    for (uint32_t i = 0; i < width; i++) {
      const double u = ((double)i + 0.5) / (double)width;
      double r, g, b;
      if (v >= 0.5) {
        const double t = (v - 0.5) * 2.0;  // horizon -> zenith
        const double s = std::sqrt(t);
        r = 0.92 + (0.22 - 0.92) * s;
        g = 0.95 + (0.42 - 0.95) * s;
        b = 1.00 + (0.85 - 1.00) * s;
        // clouds: two octaves of horizontally seamless value noise, thinning towards the zenith
        const double x = u * 24.0, y = v * 12.0;
        double c = 0.65 * value_noise(x, y, 24, 7) + 0.35 * value_noise(2.0 * x, 2.0 * y, 48, 11);
        c = (c - 0.55) * 4.0;
        if (c < 0.0) c = 0.0;
        if (c > 1.0) c = 1.0;
        c = c * (1.0 - t * 0.6);
        r = r + (1.0 - r) * c;
        g = g + (1.0 - g) * c;
        b = b + (1.0 - b) * c;
      } else {
        const double t = (0.5 - v) * 2.0;  // horizon -> nadir
        r = 0.42 - 0.22 * t;
        g = 0.38 - 0.20 * t;
        b = 0.33 - 0.18 * t;
        const double gr = value_noise(u * 96.0, v * 48.0, 96, 3);
        r = r * (0.85 + 0.3 * gr);
        g = g * (0.85 + 0.3 * gr);
        b = b * (0.85 + 0.3 * gr);
      }
      // sun disc + halo (u spans 2*pi, v spans pi: weight du by 2)
      double du = u - sun_u;
      if (du > 0.5) du -= 1.0;
      if (du < -0.5) du += 1.0;
      const double dist2 = (2.0 * du) * (2.0 * du) + (v - sun_v) * (v - sun_v);
      if (dist2 < 0.0004) {
        r = 1.0; g = 0.97; b = 0.88;
      } else {
        const double halo = 0.0012 / (dist2 + 0.0012);
        r = r + (1.0 - r) * halo * 0.8;
        g = g + (0.95 - g) * halo * 0.8;
        b = b + (0.8 - b) * halo * 0.8;
      }
      uint8_t* o = rgba + 4 * ((size_t)j * width + i);
      o[0] = quant(r);
      o[1] = quant(g);
      o[2] = quant(b);
      o[3] = 0xff;
    }
  }
  return RP_OK;
}

int rph_bvh_traversal_stats(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                            uint64_t* per_ray) {
  return rph_bvh_traversal_stats_ex(desc, rays, n, node_format, RP_COLLAPSE_AUTO, per_ray);
}

int rph_bvh_traversal_stats_ex(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                               uint32_t collapse, uint64_t* per_ray) {
  return rph_bvh_traversal_stats_opt(desc, rays, n, node_format, collapse, -1, 0, per_ray);
}

// rp_host.h's always_max and always_minor into the builder's options (always_max < 0: the builder's default)
static void always_options(int32_t always_max, uint32_t always_minor, rpb::BuildOptions& bo) {
  if (always_max >= 0) bo.always_max = (uint32_t)always_max;
  bo.always_minor = always_minor != 0;
}

int rph_bvh_traversal_stats_opt(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                                uint32_t collapse, int32_t always_max, uint32_t always_minor, uint64_t* per_ray) {
  // CPU model of rp_device.h's traversal over the same packed tree.  The arithmetic is the kernel's source: the ray
  // setup (rp_ray.h), the frame terms, plane t^ and pass test of the conservative f32 slab test and the exact f64
  // primitive tests (rp_isect.h) -- except the reciprocal, a correctly rounded 1/x for the device's v_rcp_f32.  The
  // model's own: the min/max slab form instead of the device's octant selection (the same values), one child at a
  // time, near-first order, leaf primitives tested when reached.  per_ray: n x 3 {wide nodes visited, primitive
  // tests, closest hittable id or 2^64-1}.  tests/test_bvh.py checks the closest hits against brute force.
  std::string err;
  int rc = rpb::validate(desc, err);
  if (rc != RP_OK) return fail(err);
  rpb::PackedScene ps;
  rpb::BuildOptions bo;
  bo.node_format = node_format;
  bo.collapse = collapse == RP_COLLAPSE_GREEDY ? rpb::COLLAPSE_GREEDY : rpb::COLLAPSE_SAH;
  always_options(always_max, always_minor, bo);
  rc = rpb::build(desc, bo, ps, err);
  if (rc != RP_OK) return fail(err);
  const bool q8 = ps.node_format != rpl::NODES_F32;  // Node4Q or Node8Q: the frame term
  const bool w8 = ps.node_format == rpl::NODES_W8;
  for (uint64_t r = 0; r < n; r++) {
    const double* q = rays + 8 * r;
    const rpi::V3 o = {q[0], q[1], q[2]}, d = {q[3], q[4], q[5]};
    const double tmin = q[6];
    Slabs ray;  // per axis: slope, near- and far-plane addends (rp_ray.h, as rp_device.h setup_ray32)
    for (int k = 0; k < 3; k++) {
      const rpr::Axis a =
          q8 ? rpr::axis_setup<true>(q[k], q[3 + k], ps.qbound) : rpr::axis_setup<false>(q[k], q[3 + k], 0.0);
      ray.A[k] = a.inv;
      ray.Bn[k] = a.nb;
      ray.Bf[k] = a.fb;
    }
    const float tmin32 = rpr::f32_below(tmin);
    double best = q[7];
    float best32 = rpr::best_above(best);
    int64_t bestp = -1;
    uint64_t visits = 0, tests = 0;
    auto test = [&](uint32_t k) {
      tests++;
      prim_test(ps.prims[k].kind, ps.prims[k].g, o, d, tmin, best, [&](double t, double, double) {
        best = t;
        bestp = ps.prim_refs[k].src;
        best32 = rpr::best_above(best);
      });
    };
    // the always-tested primitives first (rp_bvh.h BuildOptions::always_max), as the kernel does
    for (uint32_t k = ps.always_first; k < ps.always_first + ps.n_always; k++) test(k);
    if (w8) {
      // 8-wide: children in rank order slot ^ octant; a stack of groups {family index | imask, rank bits}; the
      // leaf children's primitives are tested when their node is visited (the kernel parks them, same hits)
      const uint32_t oct = (d.x < 0.0 ? 1u : 0u) | (d.y < 0.0 ? 2u : 0u) | (d.z < 0.0 ? 4u : 0u);
      std::vector<std::pair<uint32_t, uint32_t>> groups;  // {inner word, remaining rank bits}
      auto visit = [&](uint32_t node) {
        visits++;
        const rpl::Node8Q& nd = ps.wnodes[node];
        float tn[8];
        const uint32_t hits = children_hit(nd, frame_slabs(nd, ray), tmin32, best32, tn);
        uint32_t pm = 0;
        for (int c = 0; c < 8; c++)
          if (hits >> c & 1u) pm |= nd.pmask[c];
        for (; pm; pm &= pm - 1u) test(nd.prim + (uint32_t)__builtin_ctz(pm));
        const uint32_t ih = hits & (nd.inner >> 24);
        uint32_t ranks = 0;
        for (int c = 0; c < 8; c++)
          if (ih >> c & 1u) ranks |= 1u << (c ^ oct);
        if (ranks) groups.push_back({nd.inner, ranks});
      };
      visit(ps.root);
      while (!groups.empty()) {
        auto& g = groups.back();
        const uint32_t rk = (uint32_t)__builtin_ctz(g.second), slot = rk ^ oct, word = g.first;
        g.second &= g.second - 1u;
        if (!g.second) groups.pop_back();
        visit((word & rpl::W8_INDEX) + (uint32_t)__builtin_popcount((word >> 24) & ((1u << slot) - 1u)));
      }
    } else {
      std::vector<uint32_t> stack;
      uint32_t cur = ps.root;
      for (;;) {
        while (!(cur & rpl::ENTRY_LEAF)) {
          visits++;
          float tn[4];
          const uint32_t hits = q8 ? children_hit(ps.qnodes[cur], frame_slabs(ps.qnodes[cur], ray), tmin32, best32, tn)
                                   : children_hit(ps.nodes[cur], ray, tmin32, best32, tn);
          const uint32_t* child = q8 ? ps.qnodes[cur].child : ps.nodes[cur].child;
          uint32_t cc[4];
          for (int c = 0; c < 4; c++) {
            if (!(hits >> c & 1u) || child[c] == rpl::ENTRY_EMPTY) tn[c] = INFINITY;
            cc[c] = child[c];
          }
          for (int a = 0; a < 4; a++)  // stable sort by tn (matches the device network for distinct keys)
            for (int b = a + 1; b < 4; b++)
              if (tn[b] < tn[a]) { std::swap(tn[a], tn[b]); std::swap(cc[a], cc[b]); }
          for (int c = 3; c >= 1; c--)
            if (tn[c] != INFINITY) stack.push_back(cc[c]);
          if (tn[0] != INFINITY) cur = cc[0];
          else if (stack.empty()) cur = rpl::ENTRY_EMPTY;
          else { cur = stack.back(); stack.pop_back(); }
        }
        if (cur == rpl::ENTRY_EMPTY) break;
        const uint32_t first = cur & rpl::LEAF_FIRST_MASK, cnt = ((cur >> rpl::LEAF_SHIFT) & 7u) + 1u;
        for (uint32_t k = first; k < first + cnt; k++) test(k);
        if (stack.empty()) cur = rpl::ENTRY_EMPTY;
        else { cur = stack.back(); stack.pop_back(); }
      }
    }
    per_ray[3 * r] = visits;
    per_ray[3 * r + 1] = tests;
    per_ray[3 * r + 2] = bestp < 0 ? ~0ull : (uint64_t)bestp;
  }
  return RP_OK;
}

int rph_bvh_selfcheck(const rp_scene_desc* desc, uint32_t node_format, uint64_t* stats) {
  return rph_bvh_selfcheck_ex(desc, node_format, RP_COLLAPSE_AUTO, stats);
}

int rph_bvh_selfcheck_ex(const rp_scene_desc* desc, uint32_t node_format, uint32_t collapse, uint64_t* stats) {
  uint64_t st[6];
  const int rc = rph_bvh_selfcheck_opt(desc, node_format, collapse, -1, 0, st);
  if (rc == RP_OK && stats) std::memcpy(stats, st, 4 * sizeof(uint64_t));
  return rc;
}

int rph_bvh_selfcheck_opt(const rp_scene_desc* desc, uint32_t node_format, uint32_t collapse, int32_t always_max,
                          uint32_t always_minor, uint64_t* stats) {
  std::string err;
  int rc = rpb::validate(desc, err);
  if (rc != RP_OK) return fail(err);
  rpb::PackedScene ps;
  rpb::BuildOptions bo;
  bo.node_format = node_format;
  bo.collapse = collapse == RP_COLLAPSE_GREEDY ? rpb::COLLAPSE_GREEDY : rpb::COLLAPSE_SAH;
  always_options(always_max, always_minor, bo);
  rc = rpb::build(desc, bo, ps, err);
  if (rc != RP_OK) return fail(err);
  rc = rpb::check(ps, err);
  if (rc != RP_OK) {
    g_err = err;
    return rc;
  }
  if (stats) {
    stats[0] = ps.n_nodes();
    stats[1] = ps.n_leaves;
    stats[2] = ps.max_depth;
    stats[3] = desc->n_hittables;
    stats[4] = ps.n_always;
    stats[5] = 0;  // non-triangle primitives inside the tree (the leaf-ordered records in front of the always tail)
    for (uint32_t k = 0; k < ps.always_first; k++) stats[5] += ps.prims[k].kind != rpl::PRIM_TRIANGLE;
  }
  return RP_OK;
}

int rph_bvh_tree_hash(const rp_scene_desc* desc, uint32_t node_format, uint32_t threads, uint64_t* hash) {
  return rph_bvh_tree_hash_opt(desc, node_format, threads, -1, 0, hash);
}

int rph_bvh_tree_hash_opt(const rp_scene_desc* desc, uint32_t node_format, uint32_t threads, int32_t always_max,
                          uint32_t always_minor, uint64_t* hash) {
  std::string err;
  int rc = rpb::validate(desc, err);
  if (rc != RP_OK) return fail(err);
  rpb::PackedScene ps;
  rpb::BuildOptions bo;
  bo.node_format = node_format;
  bo.threads = threads;
  always_options(always_max, always_minor, bo);
  rc = rpb::build(desc, bo, ps, err);
  if (rc != RP_OK) return fail(err);
  uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over the packed records
  auto mix = [&](const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  };
  if (ps.node_format == rpl::NODES_W8) mix(ps.wnodes.data(), ps.wnodes.size() * sizeof(rpl::Node8Q));
  else if (ps.node_format == rpl::NODES_Q8) mix(ps.qnodes.data(), ps.qnodes.size() * sizeof(rpl::Node4Q));
  else mix(ps.nodes.data(), ps.nodes.size() * sizeof(rpl::Node4));
  mix(ps.prim_refs.data(), ps.prim_refs.size() * sizeof(rpl::PrimRef));
  *hash = h;
  return RP_OK;
}

int rph_material_head(const uint32_t fields[6], uint32_t packed[2], uint32_t unpacked[7]) {
  if (!fields || !packed || !unpacked) return fail("rph_material_head: non-NULL pointers");
  rpl::Material m{};
  m.scatter_kind = fields[0]; m.absorb_kind = fields[1]; m.emit_kind = fields[2]; m.needs_uv = fields[3];
  m.absorb_tex = fields[4]; m.emit_tex = fields[5];
  rpl::material_head_pack(m, packed[0], packed[1]);
  const rpl::MaterialHead h = rpl::material_head_unpack(packed[0], packed[1]);
  const uint32_t u[7] = {h.scatter_kind, h.absorb_kind, h.emit_kind, h.needs_uv, h.absorb_tex, h.emit_tex, h.wide ? 1u : 0u};
  for (int k = 0; k < 7; k++) unpacked[k] = u[k];
  return RP_OK;
}

int rph_scene_materials(const rp_scene_desc* desc, uint64_t cap, uint32_t* words, uint64_t* n_materials) {
  if (!desc || !n_materials || (cap && !words)) return fail("rph_scene_materials: non-NULL pointers");
  std::string err;
  int rc = rpb::validate(desc, err);
  if (rc != RP_OK) return fail(err);
  rpb::PackedScene ps;
  rpb::BuildOptions bo;
  bo.tables_only = true;
  bo.vertex_tables = false;
  rc = rpb::build(desc, bo, ps, err);
  if (rc != RP_OK) return fail(err);
  *n_materials = desc->n_materials;
  for (uint64_t i = 0; i < desc->n_materials && i < cap; i++) {
    const rpl::Material& m = ps.materials[i];
    const uint32_t w[8] = {m.scatter_kind, m.absorb_kind, m.emit_kind, m.absorb_tex, m.emit_tex, m.needs_uv, m.head, m.head_tex};
    for (int k = 0; k < 8; k++) words[8 * i + k] = w[k];
  }
  return RP_OK;
}

namespace {
inline uint32_t rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
// ChaCha12 block `ctr` of `key` (randomness.rs:5 StdRng = rand_chacha 0.3 ChaCha12Rng).
void chacha12_block(const uint32_t key[8], uint64_t ctr, uint32_t out[16]) {
  uint32_t x[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                    key[4],      key[5],      key[6],      key[7],      (uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  uint32_t s[16];
  std::memcpy(s, x, sizeof s);
  auto qr = [&](int a, int b, int c, int d) {
    x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl32(x[d], 16);
    x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl32(x[b], 12);
    x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl32(x[d], 8);
    x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl32(x[b], 7);
  };
  for (int r = 0; r < 6; r++) {
    qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
    qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
  }
  for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}
}  // namespace

int rph_stdrng_u64(const uint8_t seed[32], uint64_t first, uint64_t n, uint64_t* out) {
  if (!seed || (n && !out)) return fail("NULL argument");
  uint32_t key[8];
  for (int i = 0; i < 8; i++)
    key[i] = (uint32_t)seed[4 * i] | (uint32_t)seed[4 * i + 1] << 8 | (uint32_t)seed[4 * i + 2] << 16 |
             (uint32_t)seed[4 * i + 3] << 24;
  // draw k = words 2k, 2k+1 of the keystream = block k / 8, u64 k % 8 of it
  auto work = [&](uint64_t a, uint64_t b) {
    uint32_t w[16];
    uint64_t blk = ~0ull;
    for (uint64_t k = a; k < b; k++) {
      const uint64_t d = first + k;
      if (d / 8 != blk) {
        blk = d / 8;
        chacha12_block(key, blk, w);
      }
      const uint32_t q = (uint32_t)(d % 8);
      out[k] = (uint64_t)w[2 * q] | (uint64_t)w[2 * q + 1] << 32;
    }
  };
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const unsigned nt = n < (1u << 20) ? 1u : hw;
  std::vector<std::thread> th;
  const uint64_t per = (n + nt - 1) / nt;
  for (unsigned t = 1; t < nt; t++) {
    const uint64_t a = std::min<uint64_t>(n, t * per), b = std::min<uint64_t>(n, a + per);
    if (a < b) th.emplace_back(work, a, b);
  }
  work(0, std::min<uint64_t>(n, per));
  for (auto& t : th) t.join();
  return RP_OK;
}

int rph_make_div32(uint32_t d, uint32_t* m, uint32_t* s) {
  if (d == 0 || !m || !s) return fail("rph_make_div32: d must be >= 1 and m, s non-NULL");
  const rpk::Div32 v = rpk::make_div32(d);
  *m = v.m;
  *s = v.s;
  return RP_OK;
}

int rph_ray_setup(uint32_t node_format, double qbound, const double* rays, uint64_t n, float* out) {
  if ((node_format != RP_NODES_F32 && node_format != RP_NODES_Q8 && node_format != RP_NODES_W8) || !(qbound >= 0.0) ||
      (n && (!rays || !out)))
    return fail("rph_ray_setup: node_format f32, q8 or w8, qbound >= 0, non-NULL pointers");
  const bool frame = node_format != RP_NODES_F32;
  for (uint64_t r = 0; r < n; r++) {
    const double* q = rays + 8 * r;
    float* o = out + 11 * r;
    for (int k = 0; k < 3; k++) {
      const rpr::Axis a = frame ? rpr::axis_setup<true>(q[k], q[3 + k], qbound) : rpr::axis_setup<false>(q[k], q[3 + k], qbound);
      o[k] = a.inv;
      o[3 + k] = a.nb;
      o[6 + k] = a.fb;
    }
    o[9] = rpr::f32_below(q[6]);
    o[10] = rpr::best_above(q[7]);
  }
  return RP_OK;
}

int rph_prim_test(uint32_t kind, const double g[9], const double* rays, uint64_t n, double* out) {
  if ((kind != rpl::PRIM_SPHERE && kind != rpl::PRIM_TRIANGLE) || !g || (n && (!rays || !out)))
    return fail("rph_prim_test: kind 0 (sphere) or 1 (triangle), non-NULL pointers");
  for (uint64_t r = 0; r < n; r++) {
    const double* q = rays + 8 * r;
    double* h = out + 4 * r;
    h[0] = h[1] = h[2] = h[3] = 0.0;
    prim_test(kind, g, {q[0], q[1], q[2]}, {q[3], q[4], q[5]}, q[6], q[7], [&](double t, double u, double v) {
      h[0] = 1.0; h[1] = t; h[2] = u; h[3] = v;
    });
  }
  return RP_OK;
}

int rph_draw_round(uint32_t kind, uint32_t ring_blocks, const uint32_t* ring_image, uint32_t pos, double out[3],
                   uint32_t* new_pos, uint32_t* accepted) {
  if (kind < rpd::DRAW_SPHERE || kind > rpd::DRAW_DISK || (ring_blocks != 4 && ring_blocks != 8) || (pos & 1u) ||
      !ring_image || !out || !new_pos || !accepted)
    return fail("rph_draw_round: kind 1-4, ring_blocks 4 or 8, even pos, non-NULL pointers");
  out[0] = out[1] = out[2] = 0.0;
  // the raw image as the kernel's slab holds it: every u64 decoded where its block is made (rp_device.h ring_values)
  double held[(16u * 8u + rpd::TAIL_WORDS) / 2u];
  for (uint32_t i = 0; i < rpd::ring_image_words(ring_blocks) / 2u; i++)
    held[i] = rpd::value_store(ring_image[2 * i], ring_image[2 * i + 1]);
  if (kind == rpd::DRAW_UNIFORM) {  // the kernel's gen_f64: from the stored value at the window address
    out[0] = rpd::unit_of(held[rpd::window_word(pos, ring_blocks) >> 1]);
    *new_pos = pos + 2u;
    *accepted = 1u;
    return RP_OK;
  }
  const uint32_t stride = rpd::draw_stride(kind);
  rpd::Try t[rpd::TRIES];
  for (uint32_t j = 0; j < rpd::TRIES; j++) {  // the kernel's ring_window
    for (uint32_t k = 0; k < rpd::WINDOW_WORDS / 2u; k++) t[j].v[k] = 0.0;
    for (uint32_t k = 0; k < stride / 2u; k++) t[j].v[k] = held[rpd::value_word(pos + stride * j, k, ring_blocks) >> 1];
  }
  rpd::Draw d{0.0, 0.0, 0.0, 0.0};
  uint32_t np = pos + stride * rpd::TRIES;
  *accepted = rpd::draw_pick(stride, pos, t, d, np) ? 1u : 0u;
  *new_pos = np;
  if (*accepted) {
    if (kind == rpd::DRAW_SPHERE) {  // the Lambert site's point (rp_device.h scatter_eval)
      const double f = 2.0 * std::sqrt(1.0 - d.s);
      out[0] = d.x * f; out[1] = d.y * f; out[2] = 1.0 - 2.0 * d.s;
    } else {
      out[0] = d.x; out[1] = d.y; out[2] = d.z;
    }
  }
  return RP_OK;
}

int rph_draw_values(const uint64_t* words, uint64_t n, double* stored, double* unit) {
  if (n && (!words || !stored || !unit)) return fail("rph_draw_values: non-NULL pointers");
  for (uint64_t i = 0; i < n; i++) {
    stored[i] = rpd::value_store((uint32_t)words[i], (uint32_t)(words[i] >> 32));
    unit[i] = rpd::unit_of(stored[i]);
  }
  return RP_OK;
}

// (the hooks below take an rp_render_params field by field)
static rp_render_params scalar_params(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                                      uint32_t tile_h, uint32_t shard, uint32_t num_shards, uint32_t samples_per_stream,
                                      uint32_t shard_map) {
  rp_render_params p{};
  p.width = width;
  p.height = height;
  p.spp = spp;
  p.max_bounce = max_bounce;
  p.tile_w = tile_w;
  p.tile_h = tile_h;
  p.shard = shard;
  p.num_shards = num_shards;
  p.samples_per_stream = samples_per_stream;
  p.shard_map = shard_map;
  return p;
}

int rph_plan_launch(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w, uint32_t tile_h,
                    uint32_t shard, uint32_t num_shards, uint32_t samples_per_stream, uint32_t shard_map, uint32_t n_frames,
                    uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, uint64_t lanes, rph_launch_plan* out) {
  if (!out) return fail("rph_plan_launch: out is NULL");
  *out = rph_launch_plan{};
  const rp_render_params p = scalar_params(width, height, spp, max_bounce, tile_w, tile_h, shard, num_shards,
                                           samples_per_stream, shard_map);
  rp_scene_options opt{};
  opt.unit_queues = unit_queues;
  opt.queue_chunk = queue_chunk;
  rps::LaunchPlan lp{};
  if (!rps::make_tiling(&p, lp.t).code) {
    out->n_shard_tiles = lp.t.n_shard_tiles;
    out->nbatch = lp.t.nbatch;
    out->plan_block = rps::plan_block(lp.t.n_tiles, lp.t.shards);
    out->n_slots = lp.t.n_slots;
    out->gather_stride = rps::stage_slots(lp.t);
    out->block_words = rps::pack_words(lp.t, true, n_frames);
  }
  auto refuse = [](const rps::Refusal& r) {
    g_err = r.msg;
    return r.code;
  };
  rps::Refusal r = rps::plan_launch(&p, n_frames, frame_order, opt, lp);
  if (r.code) return refuse(r);  // nothing planned
  r = rps::launch_limits(lp, lanes);
  const rpk::KParams& kp = lp.kp;
  out->queue_groups = kp.queue_groups;
  out->queue_chunk = kp.queue_chunk;
  out->frames_inter = kp.frames_inter;
  out->sortable = lp.sortable;
  out->measure = lp.measure;
  out->grid = (uint32_t)rps::grid_for(kp.n_queue, lanes / rpk::RENDER_BLOCK);
  out->n_queue = kp.n_queue;
  out->out_stride = kp.out_stride;
  const rpk::Div32 dv[3] = {kp.dv_units, kp.dv_tiles_x, kp.dv_chunk};
  uint32_t* const dst[3] = {out->dv_units, out->dv_tiles_x, out->dv_chunk};
  for (int i = 0; i < 3; i++) {
    dst[i][0] = dv[i].m;
    dst[i][1] = dv[i].s;
  }
  return r.code ? refuse(r) : RP_OK;
}

int rph_unit_walk(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w, uint32_t tile_h,
                  uint32_t shard, uint32_t num_shards, uint32_t samples_per_stream, uint32_t shard_map, uint32_t n_frames,
                  uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, const uint32_t* tile_order,
                  const uint32_t* tile_map, const uint32_t* unit_order, uint32_t probe_lattice, uint32_t queue_groups,
                  uint32_t n_blocks, uint32_t any_every, uint32_t* units, uint64_t units_cap, uint64_t* n_units,
                  uint32_t* queue_words, uint32_t* entries, uint64_t* forced) {
  static_assert((int)RPH_QUEUE_WORDS == (int)rpk::QUEUE_WORDS, "rp_host.h states rp_kernel.h's queue words");
  if (!n_units || !queue_words || !entries || !forced || (units_cap && !units) || n_blocks == 0 ||
      queue_groups > (uint32_t)rpk::QUEUE_GROUPS)
    return fail("rph_unit_walk: NULL output, no blocks or more queues than QUEUE_GROUPS");
  const rp_render_params p = scalar_params(width, height, spp, max_bounce, tile_w, tile_h, shard, num_shards,
                                           samples_per_stream, shard_map);
  rp_scene_options opt{};
  opt.unit_queues = unit_queues;
  opt.queue_chunk = queue_chunk;
  rps::LaunchPlan lp{};
  rps::Refusal r = rps::plan_launch(&p, n_frames, frame_order, opt, lp);
  if (!r.code) r = rps::launch_limits(lp, n_blocks);
  if (r.code) {
    g_err = r.msg;
    return r.code;
  }
  const rps::Tiling& t = lp.t;
  auto below = [](const uint32_t* v, uint64_t n, uint64_t bound) {
    for (uint64_t i = 0; v && i < n; i++)
      if (v[i] >= bound) return false;
    return true;
  };
  const uint64_t shard_units = t.n_slots * t.nbatch;
  if (!below(tile_order, t.n_shard_tiles, t.n_shard_tiles) || !below(tile_map, t.n_tiles, t.n_tiles) ||
      !below(unit_order, shard_units, shard_units))
    return fail("rph_unit_walk: an order or map entry is out of range");
  UnitWalk W;
  rpk::KParams& kp = W.a.P;
  kp = lp.kp;
  if (queue_groups) kp.queue_groups = queue_groups;
  kp.tile_map = tile_map;      // rp_render.cpp balanced_plan
  kp.tile_order = tile_order;  // rp_render.cpp tile_order
  W.a.queue = W.words;         // rp_render.cpp launch_units: the workspace's queue words
  if (probe_lattice) {         // rp_render.cpp launch_probe, over the shard's tiles
    kp.probe = 1, kp.spp = 1, kp.nbatch = 1, kp.spp_batch = 1, kp.n_frames = 1;
    kp.probe_n = std::min(probe_lattice, std::min(t.tw, t.th));
    kp.probe_px = kp.probe_n * kp.probe_n;
    kp.n_queue = kp.n_slots = (uint64_t)t.n_shard_tiles * kp.probe_px;
    kp.queue_groups = 1, kp.queue_chunk = 1;
    kp.tile_order = nullptr, kp.tile_map = nullptr;
    W.a.queue = W.words + rpk::QUEUE_PROBE;
    W.probe = true;
  } else if (unit_order) {     // rp_render.cpp unit_order
    kp.unit_order = unit_order;
    kp.order_chunk = rpk::UNIT_ORDER_CHUNK;
    kp.dv_ochunk = rpk::make_div32(kp.order_chunk);
    kp.dv_tile_px = rpk::make_div32(t.tw * t.th);
  }
  auto run = [&](uint32_t* out, uint64_t cap) {
    return W.probe ? walk_units<true>(W, n_blocks, out, cap) : walk_units<false>(W, n_blocks, out, cap);
  };
  uint32_t queue_entries[rpk::QUEUE_WORDS];
  if (any_every && !W.probe) {
    // a first walk, no vote forced, counts every queue's entries: where a forced vote's wave-mate can stand
    run(nullptr, 0);
    std::memcpy(queue_entries, W.entries, sizeof queue_entries);
    const rpk::KArgs a = W.a;
    W = UnitWalk{};
    W.a = a;
    W.a.queue = W.words;
    W.any_every = any_every;
    W.queue_entries = queue_entries;
  }
  *n_units = run(units, units_cap);
  std::memcpy(queue_words, W.words, sizeof W.words);
  std::memcpy(entries, W.entries, sizeof W.entries);
  *forced = W.forced;
  if (W.err) return fail(W.err);
  if (*n_units > units_cap) return fail("rph_unit_walk: more units than units_cap");
  return RP_OK;
}

}  // extern "C"

// The denoiser's levels as a plain loop over rp_denoise.h (what rp_denoise.hip's kernel does per lane): demodulate once,
// every level from one colour buffer into the other, remodulate (or copy a pass-through pixel's rgb) at the end.
// VAR (rph_denoise_var, P an rp_denoise_var_params): the variance v travels with the colour.
template <bool VAR, class Params>
static void denoise_loop(const Params& P, uint32_t iterations, double eps, uint32_t width, uint32_t height,
                         const double* rgb, const double* var, const double* normal, const double* albedo,
                         const double* depth, double* out) {
  const uint64_t n = (uint64_t)width * height;
  std::vector<double> cur(3 * n), nxt(3 * n), vcur(VAR ? n : 0), vnxt(VAR ? n : 0);
  auto pixel = [&](const std::vector<double>& c, const std::vector<double>& v, uint64_t i) {
    rpdn::Px p = {};
    p.cx = c[3 * i], p.cy = c[3 * i + 1], p.cz = c[3 * i + 2];
    if (normal) {
      p.nx = normal[3 * i], p.ny = normal[3 * i + 1], p.nz = normal[3 * i + 2];
      p.nn = rpdn::len2(p.nx, p.ny, p.nz);
    }
    if (albedo) p.ax = albedo[3 * i], p.ay = albedo[3 * i + 1], p.az = albedo[3 * i + 2];
    if (depth) p.z = depth[i];
    if (VAR) p.v = v[i];
    return p;
  };
  for (uint64_t i = 0; i < 3 * n; i++) cur[i] = albedo ? rpdn::demod(rgb[i], albedo[i], eps) : rgb[i];
  if (VAR)
    for (uint64_t i = 0; i < n; i++) {
      double v[3];
      for (int k = 0; k < 3; k++) v[k] = albedo ? rpdn::demod_var(var[3 * i + k], albedo[3 * i + k], eps) : var[3 * i + k];
      vcur[i] = rpdn::sum3(v[0], v[1], v[2]);
    }
  rpdn::Level L{};
  for (uint32_t l = 0; l < iterations; l++) {
    L = rpdn::make_level(P, l, normal != nullptr, albedo != nullptr, depth != nullptr);
    const int64_t s = L.step;
    for (uint32_t j = 0; j < height; j++)
      for (uint32_t i = 0; i < width; i++) {
        const uint64_t at = (uint64_t)j * width + i;
        double ov = 0.0;
        rpdn::level_step_v<VAR>(
            L, pixel(cur, vcur, at),
            [&](int dx, int dy, rpdn::Px& q) {
              const int64_t qi = (int64_t)i + s * dx, qj = (int64_t)j + s * dy;
              if (qi < 0 || qi >= (int64_t)width || qj < 0 || qj >= (int64_t)height) return false;
              q = pixel(cur, vcur, (uint64_t)qj * width + (uint64_t)qi);
              return true;
            },
            nxt[3 * at], nxt[3 * at + 1], nxt[3 * at + 2], ov);
        if (VAR) vnxt[at] = ov;
      }
    cur.swap(nxt);
    vcur.swap(vnxt);
  }
  for (uint64_t at = 0; at < n; at++) {
    const rpdn::Px p = pixel(cur, vcur, at);
    for (int k = 0; k < 3; k++) {
      const uint64_t i = 3 * at + k;
      out[i] = rpdn::passes(L, p) ? rgb[i] : (albedo ? rpdn::remod(cur[i], albedo[i], eps) : cur[i]);
    }
  }
}

// What rph_denoise and rph_denoise_var refuse about their frames (var NULL: the former); NULL = fine.
static const char* denoise_frames(uint32_t width, uint32_t height, const double* rgb, const double* var,
                                  const double* normal, const double* albedo, const double* depth, const double* out) {
  if (width == 0 || height == 0 || width > 65535 || height > 65535) return "width and height must be 1..65535";
  if (!rgb || !out) return "rgb and out must be non-NULL";
  const uint64_t n = (uint64_t)width * height;
  auto overlaps = [&](const double* in, uint64_t channels) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(out), y = reinterpret_cast<uintptr_t>(in);
    return in && x < y + 8 * channels * n && y < x + 24 * n;
  };
  if (overlaps(rgb, 3) || overlaps(normal, 3) || overlaps(albedo, 3) || overlaps(depth, 1) || overlaps(var, 3))
    return "out must not alias an input";
  return nullptr;
}

extern "C" {

int rph_denoise(const rp_denoise_params* params, uint32_t width, uint32_t height, const double* rgb, const double* normal,
                const double* albedo, const double* depth, double* out) {
  if (const char* why = denoise_frames(width, height, rgb, nullptr, normal, albedo, depth, out))
    return fail(std::string("rph_denoise: ") + why);
  rp_denoise_params P;
  if (!rpdn::resolve(params, P))
    return fail("rph_denoise: params out of range (iterations 1..8, normal_power 1..8, sigma_depth, sigma_albedo and "
                "albedo_eps > 0 and finite, sigma_color finite)");
  denoise_loop<false>(P, P.iterations, P.albedo_eps, width, height, rgb, nullptr, normal, albedo, depth, out);
  return RP_OK;
}

int rph_denoise_var(const rp_denoise_var_params* params, uint32_t width, uint32_t height, const double* rgb,
                    const double* var, const double* normal, const double* albedo, const double* depth, double* out) {
  if (const char* why = denoise_frames(width, height, rgb, var, normal, albedo, depth, out))
    return fail(std::string("rph_denoise_var: ") + why);
  if (!var) return fail("rph_denoise_var: var must be non-NULL");
  rp_denoise_var_params P;
  if (!rpdn::resolve(params, P))
    return fail("rph_denoise_var: params out of range (iterations 1..8, normal_power 1..8, sigma_depth, sigma_albedo, "
                "albedo_eps, sigma_var and var_eps > 0 and finite)");
  denoise_loop<true>(P, P.base.iterations, P.base.albedo_eps, width, height, rgb, var, normal, albedo, depth, out);
  return RP_OK;
}

// rp_variance.h's batch_variance per pixel and channel: what rp_variance.hip's kernel does per lane.
int rph_batch_variance(uint32_t spp, uint32_t samples_per_stream, uint64_t n_pixels, const double* sums, double* var) {
  if (!sums || !var) return fail("rph_batch_variance: sums and var must be non-NULL");
  const uint32_t sps = samples_per_stream ? samples_per_stream : RP_SAMPLES_PER_STREAM;
  const uint32_t B = rpv::batches(spp, sps);
  if (B < 2) return fail("rph_batch_variance: needs at least two sample batches per pixel (spp > samples_per_stream)");
  for (uint64_t i = 0; i < n_pixels; i++)
    for (uint32_t c = 0; c < 3; c++) var[3 * i + c] = rpv::batch_variance(sums + 3 * i * B + c, 3, B, spp, sps);
  return RP_OK;
}

// rp_accum.h's Welford update per word, frame after frame: what rp_accum.hip's accum_kernel does per lane.
int rph_accum_frames(uint64_t n_words, uint32_t n_prior, uint32_t n_frames, const double* frames, uint64_t frame_stride,
                     double* mean, double* m2, double* var) {
  if (!frames || !mean || !m2) return fail("rph_accum_frames: frames, mean and m2 must be non-NULL");
  if (n_words == 0) return fail("rph_accum_frames: n_words is zero");
  if (n_frames == 0) return fail("rph_accum_frames: n_frames is zero: nothing to fold in");
  if (frame_stride < n_words) return fail("rph_accum_frames: frame_stride is below n_words: the frames would overlap");
  const uint64_t n = (uint64_t)n_prior + n_frames;
  if (n > 0x7fffffffu) return fail("rph_accum_frames: more than 2^31 - 1 frames (n_prior + n_frames)");
  if (var && n < 2) return fail("rph_accum_frames: the variance needs at least two frames (n_prior + n_frames >= 2)");
  if (n_words > (1ull << 40) - 512) return fail("rph_accum_frames: n_words is above 2^40 - 512");
  const uint64_t in_bytes = 8 * ((uint64_t)(n_frames - 1) * frame_stride + n_words), out_bytes = 8 * n_words;
  auto overlaps = [](const double* a, uint64_t na, const double* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
  };
  if (overlaps(mean, out_bytes, frames, in_bytes) || overlaps(m2, out_bytes, frames, in_bytes) ||
      overlaps(var, out_bytes, frames, in_bytes))
    return fail("rph_accum_frames: mean, m2 and var must not alias the frames");
  if (overlaps(mean, out_bytes, m2, out_bytes) || overlaps(var, out_bytes, mean, out_bytes) ||
      overlaps(var, out_bytes, m2, out_bytes))
    return fail("rph_accum_frames: mean, m2 and var must not alias one another");
  if (!n_prior)
    for (uint64_t w = 0; w < n_words; w++) mean[w] = 0.0, m2[w] = 0.0;
  for (uint32_t f = 0; f < n_frames; f++) {
    const double r = rpa::frame_weight(n_prior + f + 1);
    const double* x = frames + (uint64_t)f * frame_stride;
    for (uint64_t w = 0; w < n_words; w++) rpa::welford(x[w], r, mean[w], m2[w]);
  }
  if (var) {
    const double nn = rpa::mean_divisor((uint32_t)n);
    for (uint64_t w = 0; w < n_words; w++) var[w] = rpa::mean_variance(m2[w], nn);
  }
  return RP_OK;
}

// rp_accum.h's error2 per pixel and the four order-free statistics: what rp_accum.hip's error_kernel reduces.
int rph_accum_error(const rp_error_params* params, uint64_t n_pixels, const double* mean, const double* var,
                    uint64_t* stats) {
  if (!mean || !var || !stats) return fail("rph_accum_error: mean, var and stats must be non-NULL");
  double tol, eps;
  if (!rpa::resolve(params, tol, eps))
    return fail("rph_accum_error: error params out of range (tol > 0; eps > 0 and finite)");
  const double tol2 = tol * tol;
  for (int k = 0; k < rpa::STATS_LEN; k++) stats[k] = 0;
  for (uint64_t i = 0; i < n_pixels; i++) {
    const double e2 = rpa::error2(mean + 3 * i, var + 3 * i, eps);
    stats[rpa::STAT_PIXELS]++;
    if (e2 > tol2) stats[rpa::STAT_OVER]++;
    if (!rpa::finite(e2)) {
      stats[rpa::STAT_NONFINITE]++;
    } else if (e2 > 0.0) {
      uint64_t bits;
      std::memcpy(&bits, &e2, sizeof bits);
      if (bits > stats[rpa::STAT_MAX_BITS]) stats[rpa::STAT_MAX_BITS] = bits;
    }
  }
  return RP_OK;
}

// rp_accum_frames_tiles_device on host buffers: rph_accum_frames' loop per listed block, an entry at or above
// n_state_tiles skipped (what rp_accum.hip's accum_tiles_kernel does per lane).
int rph_accum_frames_tiles(uint64_t tile_words, uint32_t n_state_tiles, const uint32_t* tiles, uint32_t n_listed,
                           uint32_t n_prior, uint32_t n_frames, const double* frames, uint64_t frame_stride, double* mean,
                           double* m2, double* var) {
  if (!frames || !mean || !m2) return fail("rph_accum_frames_tiles: frames, mean and m2 must be non-NULL");
  if (tile_words == 0) return fail("rph_accum_frames_tiles: tile_words is zero");
  if (n_frames == 0) return fail("rph_accum_frames_tiles: n_frames is zero: nothing to fold in");
  if (n_listed > n_state_tiles) return fail("rph_accum_frames_tiles: n_listed is above n_state_tiles");
  if (n_listed && !tiles) return fail("rph_accum_frames_tiles: tiles must be non-NULL");
  if (tile_words > (1ull << 40) - 512 || (uint64_t)n_state_tiles * tile_words > (1ull << 40) - 512)
    return fail("rph_accum_frames_tiles: the state is above 2^40 - 512 words (n_state_tiles * tile_words)");
  const uint64_t n_words = (uint64_t)n_listed * tile_words, n_state = (uint64_t)n_state_tiles * tile_words;
  if (frame_stride < n_words)
    return fail("rph_accum_frames_tiles: frame_stride is below n_listed * tile_words: the frames would overlap");
  const uint64_t n = (uint64_t)n_prior + n_frames;
  if (n > 0x7fffffffu) return fail("rph_accum_frames_tiles: more than 2^31 - 1 frames (n_prior + n_frames)");
  if (var && n < 2) return fail("rph_accum_frames_tiles: the variance needs at least two frames (n_prior + n_frames >= 2)");
  if (n_listed == 0) return RP_OK;
  const uint64_t in_bytes = 8 * ((uint64_t)(n_frames - 1) * frame_stride + n_words), out_bytes = 8 * n_state;
  auto overlaps = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
  };
  for (const double* o : {(const double*)mean, (const double*)m2, (const double*)var})
    if (overlaps(o, out_bytes, frames, in_bytes) || overlaps(o, out_bytes, tiles, 4ull * n_listed))
      return fail("rph_accum_frames_tiles: mean, m2 and var must not alias the frames or the list");
  if (overlaps(mean, out_bytes, m2, out_bytes) || overlaps(var, out_bytes, mean, out_bytes) ||
      overlaps(var, out_bytes, m2, out_bytes))
    return fail("rph_accum_frames_tiles: mean, m2 and var must not alias one another");
  const double nn = var ? rpa::mean_divisor((uint32_t)n) : 0.0;
  for (uint32_t k = 0; k < n_listed; k++) {
    if (tiles[k] >= n_state_tiles) continue;
    double* mk = mean + (uint64_t)tiles[k] * tile_words;
    double* qk = m2 + (uint64_t)tiles[k] * tile_words;
    if (!n_prior)
      for (uint64_t w = 0; w < tile_words; w++) mk[w] = 0.0, qk[w] = 0.0;
    for (uint32_t f = 0; f < n_frames; f++) {
      const double r = rpa::frame_weight(n_prior + f + 1);
      const double* x = frames + (uint64_t)f * frame_stride + (uint64_t)k * tile_words;
      for (uint64_t w = 0; w < tile_words; w++) rpa::welford(x[w], r, mk[w], qk[w]);
    }
    if (var) {
      double* vk = var + (uint64_t)tiles[k] * tile_words;
      for (uint64_t w = 0; w < tile_words; w++) vk[w] = rpa::mean_variance(qk[w], nn);
    }
  }
  return RP_OK;
}

// rp_accum_tiles_select_device on host buffers: rp_accum.h's pixel_over per in-frame pixel of every listed tile, the
// tile's count, tile_active, and the active tiles in list order (what rp_tiles.hip's two kernels do).
int rph_accum_tiles_select(const rp_render_params* params, const rp_error_params* error, double tile_share,
                           const double* mean, const double* var, const uint32_t* tiles_in, uint32_t n_in, uint32_t* over,
                           uint32_t* tiles_out, uint32_t* count) {
  if (!mean || !var || !tiles_out || !count)
    return fail("rph_accum_tiles_select: mean, var, tiles_out and count must be non-NULL");
  rps::Tiling t;
  const rps::Refusal r = rps::make_tiling(params, t);
  if (r.code) return fail(std::string("rph_accum_tiles_select: ") + r.msg);
  if (t.shards != 1 || params->shard_map != RP_SHARD_INTERLEAVE)
    return fail("rph_accum_tiles_select: the state is a whole frame's: num_shards 0 or 1, shard 0, interleave");
  double tol, eps;
  if (!rpa::resolve(error, tol, eps))
    return fail("rph_accum_tiles_select: error params out of range (tol > 0; eps > 0 and finite)");
  if (!(tile_share >= 0.0 && tile_share < 1.0)) return fail("rph_accum_tiles_select: tile_share must be in [0, 1)");
  if (n_in > (uint32_t)rpk::TILE_SORT_MAX) return fail("rph_accum_tiles_select: n_in is above 16384 (rpk::TILE_SORT_MAX)");
  const double tol2 = tol * tol;
  const uint32_t W = params->width, H = params->height, tile_px = t.tw * t.th;
  uint32_t n_out = 0;
  for (uint32_t k = 0; k < n_in; k++) {
    const uint32_t tile = tiles_in ? tiles_in[k] : k;
    uint32_t n_over = 0;
    const bool in_frame = tile < t.n_tiles;
    if (in_frame) {
      const uint32_t ox = (tile % t.tiles_x) * t.tw, oy = (tile / t.tiles_x) * t.th;
      for (uint32_t lj = 0; lj < t.th && oy + lj < H; lj++)
        for (uint32_t li = 0; li < t.tw && ox + li < W; li++) {
          const uint64_t slot = (uint64_t)tile * tile_px + (uint64_t)lj * t.tw + li;
          n_over += rpa::pixel_over(mean + 3 * slot, var + 3 * slot, eps, tol2);
        }
    }
    if (over) over[k] = n_over;
    // (tiles_out may be tiles_in here: position n_out is never beyond entry k, which has been read)
    if (in_frame && rpa::tile_active(n_over, rpa::tile_pixels(tile, W, H, t.tw, t.th, t.tiles_x), tile_share))
      tiles_out[n_out++] = tile;
  }
  count[0] = n_out;
  return RP_OK;
}

// rp_reproject.h's reproject_pixel per pixel and the four order-free statistics: what rp_reproject.hip's kernel does
// per lane and reduces.
int rph_reproject(const rp_reproject_params* params, uint32_t width, uint32_t height, const rp_camera* cur,
                  const rp_camera* prev, const double* depth_cur, const double* normal_cur, const double* depth_prev,
                  const double* normal_prev, const double* mean_prev, const double* m2_prev, const uint32_t* count_prev,
                  double* mean, double* m2, uint32_t* count, uint64_t* stats) {
  if (!cur || !prev) return fail("rph_reproject: cur and prev must be non-NULL");
  if (const char* why = rprj::check_buffers(width, height, depth_cur, normal_cur, depth_prev, normal_prev, mean_prev,
                                            m2_prev, count_prev, mean, m2, count, stats))
    return fail(std::string("rph_reproject: ") + why);
  rprj::Frame F;
  if (!rprj::resolve(params, F.P))
    return fail("rph_reproject: params out of range (sigma_depth > 0 and finite, normal_cos in (0, 1], max_history "
                "1 .. 2^31 - 1)");
  if (!rprj::make_camera(*cur, F.cur) || !rprj::make_camera(*prev, F.prev))
    return fail("rph_reproject: a camera field is not finite, or tan(fov / 2) is not > 0");
  F.W = width, F.H = height;
  F.depth_prev = depth_prev, F.normal_prev = normal_prev;
  F.mean_prev = mean_prev, F.m2_prev = m2_prev, F.count_prev = count_prev;
  for (int k = 0; k < rprj::STATS_LEN; k++) stats[k] = 0;
  for (uint32_t j = 0; j < height; j++)
    for (uint32_t i = 0; i < width; i++) {
      const uint64_t px = (uint64_t)j * width + i;
      const rprj::Result r = rprj::reproject_pixel(F, i, j, depth_cur[px], normal_cur[3 * px], normal_cur[3 * px + 1],
                                                   normal_cur[3 * px + 2]);
      for (int ch = 0; ch < 3; ch++) mean[3 * px + ch] = r.mean[ch], m2[3 * px + ch] = r.m2[ch];
      count[px] = r.count;
      stats[rprj::STAT_PIXELS]++;
      stats[rprj::STAT_KEPT] += r.count >= 1;
      stats[rprj::STAT_COUNT] += r.count;
      stats[rprj::STAT_OFF] += r.off;
    }
  return RP_OK;
}

// rp_accum.h's Welford update with the frame number taken per pixel: what rp_accum.hip's accum_counts_kernel does per
// lane.
int rph_accum_frames_counts(uint64_t n_pixels, uint32_t words_per_pixel, uint32_t n_frames, const double* frames,
                            uint64_t frame_stride, uint32_t* count, double* mean, double* m2, double* var, double var_one) {
  if (!frames || !mean || !m2 || !count)
    return fail("rph_accum_frames_counts: frames, count, mean and m2 must be non-NULL");
  if (n_pixels == 0 || words_per_pixel == 0) return fail("rph_accum_frames_counts: n_pixels or words_per_pixel is zero");
  if (n_frames == 0) return fail("rph_accum_frames_counts: n_frames is zero: nothing to fold in");
  if (n_frames > 0x7fffffffu) return fail("rph_accum_frames_counts: more than 2^31 - 1 frames");
  if (n_pixels > ((1ull << 40) - 512) / words_per_pixel)
    return fail("rph_accum_frames_counts: n_pixels * words_per_pixel is above 2^40 - 512");
  const uint64_t n_words = n_pixels * words_per_pixel;
  if (frame_stride < n_words)
    return fail("rph_accum_frames_counts: frame_stride is below n_pixels * words_per_pixel: the frames would overlap");
  if (!(var_one >= 0.0 && rpa::finite(var_one))) return fail("rph_accum_frames_counts: var_one must be finite and >= 0");
  const uint64_t in_bytes = 8 * ((uint64_t)(n_frames - 1) * frame_stride + n_words), out_bytes = 8 * n_words;
  auto overlaps = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
  };
  if (overlaps(mean, out_bytes, frames, in_bytes) || overlaps(m2, out_bytes, frames, in_bytes) ||
      overlaps(var, out_bytes, frames, in_bytes))
    return fail("rph_accum_frames_counts: mean, m2 and var must not alias the frames");
  if (overlaps(mean, out_bytes, m2, out_bytes) || overlaps(var, out_bytes, mean, out_bytes) ||
      overlaps(var, out_bytes, m2, out_bytes))
    return fail("rph_accum_frames_counts: mean, m2 and var must not alias one another");
  if (overlaps(count, 4 * n_pixels, frames, in_bytes) || overlaps(count, 4 * n_pixels, mean, out_bytes) ||
      overlaps(count, 4 * n_pixels, m2, out_bytes) || overlaps(count, 4 * n_pixels, var, out_bytes))
    return fail("rph_accum_frames_counts: count must not alias the frames or the state");
  for (uint64_t p = 0; p < n_pixels; p++) {
    const uint32_t c = count[p], n = c + n_frames;
    double* mp = mean + p * words_per_pixel;
    double* qp = m2 + p * words_per_pixel;
    if (!c)
      for (uint32_t w = 0; w < words_per_pixel; w++) mp[w] = 0.0, qp[w] = 0.0;
    for (uint32_t f = 0; f < n_frames; f++) {
      const double r = rpa::frame_weight(c + f + 1);
      const double* x = frames + (uint64_t)f * frame_stride + p * words_per_pixel;
      for (uint32_t w = 0; w < words_per_pixel; w++) rpa::welford(x[w], r, mp[w], qp[w]);
    }
    if (var) {
      const double nn = rpa::mean_divisor(n);
      for (uint32_t w = 0; w < words_per_pixel; w++)
        var[p * words_per_pixel + w] = n >= 2 ? rpa::mean_variance(qp[w], nn) : var_one;
    }
    count[p] = n;
  }
  return RP_OK;
}

// The plan of a tile-list launch (rp_schedule.h rps::plan_tiles_launch, what rp_render_tiles_device_ws launches with).
static rps::Refusal tiles_plan(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                               uint32_t tile_h, uint32_t samples_per_stream, uint32_t n_listed, uint32_t n_frames,
                               uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, uint64_t lanes,
                               rps::LaunchPlan& lp, bool& planned) {
  const rp_render_params p = scalar_params(width, height, spp, max_bounce, tile_w, tile_h, 0, 1, samples_per_stream,
                                           RP_SHARD_INTERLEAVE);
  rp_scene_options opt{};
  opt.unit_queues = unit_queues;
  opt.queue_chunk = queue_chunk;
  planned = false;
  rps::Refusal r = rps::plan_tiles_launch(&p, n_listed, n_frames, frame_order, opt, lp);
  if (r.code) return r;
  planned = true;
  return rps::launch_limits(lp, lanes);
}

int rph_plan_tiles_launch(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                          uint32_t tile_h, uint32_t samples_per_stream, uint32_t n_listed, uint32_t n_frames,
                          uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, uint64_t lanes,
                          rph_launch_plan* out) {
  if (!out) return fail("rph_plan_tiles_launch: out is NULL");
  *out = rph_launch_plan{};
  rps::LaunchPlan lp{};
  bool planned;
  const rps::Refusal r = tiles_plan(width, height, spp, max_bounce, tile_w, tile_h, samples_per_stream, n_listed, n_frames,
                                    frame_order, unit_queues, queue_chunk, lanes, lp, planned);
  if (planned) {
    const rpk::KParams& kp = lp.kp;
    out->n_shard_tiles = lp.t.n_shard_tiles;
    out->nbatch = lp.t.nbatch;
    out->plan_block = 1;
    out->n_slots = lp.t.n_slots;
    out->queue_groups = kp.queue_groups;
    out->queue_chunk = kp.queue_chunk;
    out->frames_inter = kp.frames_inter;
    out->sortable = lp.sortable;
    out->measure = lp.measure;
    out->grid = (uint32_t)rps::grid_for(kp.n_queue, lanes / rpk::RENDER_BLOCK);
    out->n_queue = kp.n_queue;
    out->out_stride = kp.out_stride;
    const rpk::Div32 dv[3] = {kp.dv_units, kp.dv_tiles_x, kp.dv_chunk};
    uint32_t* const dst[3] = {out->dv_units, out->dv_tiles_x, out->dv_chunk};
    for (int i = 0; i < 3; i++) dst[i][0] = dv[i].m, dst[i][1] = dv[i].s;
  }
  if (r.code) {
    g_err = r.msg;
    return r.code;
  }
  return RP_OK;
}

int rph_tiles_unit_walk(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                        uint32_t tile_h, uint32_t samples_per_stream, uint32_t n_frames, uint32_t frame_order,
                        uint32_t unit_queues, uint32_t queue_chunk, const uint32_t* tiles, uint32_t n_listed,
                        uint32_t n_blocks, uint32_t* units, uint64_t units_cap, uint64_t* n_units, uint32_t* queue_words,
                        uint32_t* entries) {
  if (!n_units || !queue_words || !entries || (units_cap && !units) || n_blocks == 0 || (n_listed && !tiles))
    return fail("rph_tiles_unit_walk: NULL list or output, or no blocks");
  rps::LaunchPlan lp{};
  bool planned;
  const rps::Refusal r = tiles_plan(width, height, spp, max_bounce, tile_w, tile_h, samples_per_stream, n_listed, n_frames,
                                    frame_order, unit_queues, queue_chunk, n_blocks, lp, planned);
  if (r.code) {
    g_err = r.msg;
    return r.code;
  }
  UnitWalk W;
  W.a.P = lp.kp;
  W.a.P.tile_map = tiles;  // rp_tiles.hip: the list is the one-shard launch's tile map
  W.a.queue = W.words;
  *n_units = n_listed ? walk_units<false>(W, n_blocks, units, units_cap) : 0;
  std::memcpy(queue_words, W.words, sizeof W.words);
  std::memcpy(entries, W.entries, sizeof W.entries);
  if (W.err) return fail(W.err);
  if (*n_units > units_cap) return fail("rph_tiles_unit_walk: more units than units_cap");
  return RP_OK;
}

}  // extern "C"
