// volume.hip -- the 3-D segmentation stages (biofilm_analysis.py:818-859, :489-499): connected
// components, cross-footprint morphology, fill-holes, small-object removal and the watershed on
// (X, Y, Z) volumes.  The volume's layout and limit and the 4 x 4 x 64 brick are vol.hpp's.
//
// Components: label.hip's three passes with the brick in place of the 32 x 32 tile and the same
// union-find (cc_core.hpp): in LDS per brick, the brick-crossing pairs merged in global memory,
// then compression; parent[p] = the component's minimum raster index.  Numbering, sizes and
// relabelling are label.hip's own entry points, which are flat in n.
//
// The watershed is watershed.hip's on the 6-neighbour graph, by the same rule (ws_core.hpp: order,
// initial state, transition): the relaxation of (lambda, hop, basin distance, label) in LDS bricks
// with ping-pong passes, then a count of the voxels whose least-key labelled neighbours carry
// different labels (ws3_contest_kernel).  None: the relaxation's labels are the heap flood's (the
// order theorem of DESIGN.md "Watershed" is stated on the neighbour graph).  Any: the volume is
// flooded by the one-workgroup heap kernel (watershed.hip, six neighbours in raster-offset order
// -X, -Y, -Z, +Z, +Y, +X) and its labels are returned; there is no 3-D string-walk resolver.
#include <algorithm>

#include "cc_core.hpp"
#include "detmath.h"
#include "vol.hpp"
#include "wave.hpp"
#include "ws_core.hpp"

namespace {

using namespace hrf_cc;
using namespace hrf_vol;
using namespace hrf_ws;

// the 13 neighbour offsets that precede a voxel in raster order, fewest non-zero components
// first within each connectivity class: CONN 1 uses the first 3, CONN 2 the first 9, CONN 3 all
__constant__ int8_t PREV_OFF[13][3] = {
    {-1, 0, 0}, {0, -1, 0}, {0, 0, -1},                                                      // faces
    {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1}, {-1, 0, 1}, {0, -1, -1}, {0, -1, 1},               // edges
    {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};                                     // corners
__host__ __device__ constexpr int prev_count(int conn) { return conn == 1 ? 3 : conn == 2 ? 9 : 13; }

// One workgroup per brick.  Local index li = (lx * BY + ly) * BZ + lz runs in the raster order of
// the volume, so a brick-local root (the least local index) is the least raster index too.
template <class V, int CONN>
__global__ __launch_bounds__(256) void cc3_local_kernel(V val, Vol g, int nby, int nbz, int32_t *__restrict__ parent) {
  __shared__ int32_t lp[BV];
  __shared__ int32_t lv[BV];
  const int tid = threadIdx.x;
  const Brick bk = brick_of((int64_t)blockIdx.x, nby, nbz);
  const int64_t x0 = bk.x0(), y0 = bk.y0(), z0 = bk.z0();
  const int ly = tid >> 6, lz = tid & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int li = tid + 256 * k;  // lx = k
    const int64_t gx = x0 + k, gy = y0 + ly, gz = z0 + lz;
    const int32_t v = (gx < g.X && gy < g.Y && gz < g.Z) ? val((gx * g.Y + gy) * g.Z + gz) : 0;
    lv[li] = v;
    lp[li] = v ? li : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int li = tid + 256 * k;
    const int32_t v = lv[li];
    if (!v) continue;
#pragma unroll
    for (int o = 0; o < prev_count(CONN); ++o) {
      const int qx = k + PREV_OFF[o][0], qy = ly + PREV_OFF[o][1], qz = lz + PREV_OFF[o][2];
      if (qx < 0 || qy < 0 || qy >= BY || qz < 0 || qz >= BZ) continue;
      const int lj = (qx * BY + qy) * BZ + qz;
      if (lv[lj] == v) union_lds(lp, li, lj);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int li = tid + 256 * k;
    const int64_t gx = x0 + k, gy = y0 + ly, gz = z0 + lz;
    if (gx >= g.X || gy >= g.Y || gz >= g.Z) continue;
    int32_t r = -1;
    if (lv[li]) {
      const int rt = find_lds(lp, li);
      r = (int32_t)(((x0 + (rt >> 8)) * g.Y + y0 + ((rt >> 6) & 3)) * g.Z + z0 + (rt & 63));
    }
    parent[(gx * g.Y + gy) * g.Z + gz] = r;
  }
}

// The pairs (voxel, preceding neighbour) that cross a brick boundary, merged in global memory.
// Reads may be stale; atomicMin's returned value makes the union exact (cc_core.hpp).
template <class V, int CONN>
__global__ void cc3_border_kernel(V val, Vol g, int32_t *__restrict__ parent) {
  const int64_t n = g.n();
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t z = p % g.Z, y = (p / g.Z) % g.Y, x = p / (g.Z * g.Y);
    const int lx = (int)(x % BX), ly = (int)(y % BY), lz = (int)(z % BZ);
    // a preceding neighbour lies in another brick only from these local positions
    if (lx > 0 && ly > 0 && ly < BY - 1 && lz > 0 && lz < BZ - 1) continue;
    const int32_t v = val(p);
    if (!v) continue;
    for (int o = 0; o < prev_count(CONN); ++o) {
      const int dx = PREV_OFF[o][0], dy = PREV_OFF[o][1], dz = PREV_OFF[o][2];
      const int64_t qx = x + dx, qy = y + dy, qz = z + dz;
      if (qx < 0 || qy < 0 || qy >= g.Y || qz < 0 || qz >= g.Z) continue;
      const int jx = lx + dx, jy = ly + dy, jz = lz + dz;
      if (jx >= 0 && jy >= 0 && jy < BY && jz >= 0 && jz < BZ) continue;  // same brick: done in LDS
      const int64_t q = (qx * g.Y + qy) * g.Z + qz;
      if (val(q) == v) union_g(parent, (int32_t)p, (int32_t)q);
    }
  }
}

// every store is a root, so concurrent finds stay valid (label.hip cc_compress_kernel)
__global__ void cc3_compress_kernel(int32_t *__restrict__ parent, int64_t n) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t q = parent[p];
    if (q >= 0 && q != p) parent[p] = find_g(parent, q);
  }
}

template <class V>
hrf_status run_cc3(V val, Vol g, int conn, int32_t *parent, hipStream_t s) {
  const unsigned nb = (unsigned)g.bricks();
  const int nby = (int)g.by(), nbz = (int)g.bz();
  const unsigned sg = hrf::stream_grid(g.n());
  switch (conn) {
    case 1:
      cc3_local_kernel<V, 1><<<nb, 256, 0, s>>>(val, g, nby, nbz, parent);
      cc3_border_kernel<V, 1><<<sg, 256, 0, s>>>(val, g, parent);
      break;
    case 2:
      cc3_local_kernel<V, 2><<<nb, 256, 0, s>>>(val, g, nby, nbz, parent);
      cc3_border_kernel<V, 2><<<sg, 256, 0, s>>>(val, g, parent);
      break;
    default:
      cc3_local_kernel<V, 3><<<nb, 256, 0, s>>>(val, g, nby, nbz, parent);
      cc3_border_kernel<V, 3><<<sg, 256, 0, s>>>(val, g, parent);
  }
  cc3_compress_kernel<<<sg, 256, 0, s>>>(parent, g.n());
  HRF_LAUNCHED();
  return HRF_OK;
}

__global__ void keep3_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ size, int64_t n,
                             int64_t thr, uint8_t *__restrict__ out) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t q = parent[p];
    out[p] = (uint8_t)(q >= 0 && (int64_t)size[q] >= thr);
  }
}

// flag[root] = 1 for the background components with a voxel on one of the volume's six faces
__global__ void face_roots3_kernel(const int32_t *__restrict__ parent, Vol g, int32_t *__restrict__ flag) {
  const int64_t n = g.n();
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t z = p % g.Z, y = (p / g.Z) % g.Y, x = p / (g.Z * g.Y);
    if (x != 0 && y != 0 && z != 0 && x != g.X - 1 && y != g.Y - 1 && z != g.Z - 1) continue;
    const int32_t q = parent[p];
    if (q >= 0) flag[q] = 1;
  }
}

__global__ void fill3_finish_kernel(const uint8_t *__restrict__ mask, const int32_t *__restrict__ parent,
                                    const int32_t *__restrict__ flag, int64_t n, uint8_t *__restrict__ out) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t q = parent[p];  // component of the background
    out[p] = (uint8_t)(mask[p] != 0 || (q >= 0 && !flag[q]));
  }
}

// ---- morphology, 6-neighbour cross ----------------------------------------------------------
template <bool ERODE>
__global__ void morph3_kernel(const uint8_t *__restrict__ m, Vol g, int border, uint8_t *__restrict__ o) {
  const int64_t n = g.n(), sy = g.Z, sx = g.Y * g.Z;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t z = p % g.Z, y = (p / g.Z) % g.Y, x = p / sx;
    // outside the volume: the border value for the erosion, 0 for the dilation
    const int out = ERODE ? border : 0;
    const int a = x > 0 ? m[p - sx] != 0 : out, b = x + 1 < g.X ? m[p + sx] != 0 : out;
    const int c = y > 0 ? m[p - sy] != 0 : out, d = y + 1 < g.Y ? m[p + sy] != 0 : out;
    const int e = z > 0 ? m[p - 1] != 0 : out, f = z + 1 < g.Z ? m[p + 1] != 0 : out;
    const int self = m[p] != 0;
    o[p] = (uint8_t)(ERODE ? (self & a & b & c & d & e & f) : (self | a | b | c | d | e | f));
  }
}

// log10(x + 1) with the correctly rounded log10 of channel_sum's mode 2 (biofilm :845)
__global__ void log10p1_kernel(const double *__restrict__ x, int64_t n, double *__restrict__ o) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
    o[p] = hrf_cr_log10(x[p] + 1.0);
}

// ---- watershed relaxation -------------------------------------------------------------------
struct WsState {
  double *lam;
  int32_t *hop;
  int32_t *lab;
  int32_t *dst;  // basin distance (relaxation tie-break only, watershed.hip ws_pass_kernel)
};

// flags: [0] change flag of a batch's last pass, [1] the other passes', [2] contested voxels,
// [3] 1 when a voxel the relaxation can change exists (in the mask and not a marker)
__global__ __launch_bounds__(256) void ws3_init_kernel(const double *__restrict__ f, int negate,
                                                       const int32_t *__restrict__ markers,
                                                       const uint8_t *__restrict__ mask, Vol g, int nby, int nbz,
                                                       WsState a, WsState b, int32_t *__restrict__ brick_work,
                                                       int32_t *__restrict__ brick_marker,
                                                       int32_t *__restrict__ brick_flags,
                                                       int32_t *__restrict__ flags) {
  const int tid = threadIdx.x;
  const int64_t nbr = gridDim.x, br = blockIdx.x;
  if (tid < 2) brick_flags[tid * nbr + br] = 0;  // change flags of generations 0 and 1
  const Brick bk = brick_of(br, nby, nbz);
  const int64_t x0 = bk.x0(), y0 = bk.y0(), z0 = bk.z0();
  const int ly = tid >> 6, lz = tid & 63;
  int work = 0, mark = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t gx = x0 + k, gy = y0 + ly, gz = z0 + lz;
    if (gx >= g.X || gy >= g.Y || gz >= g.Z) continue;
    const int64_t i = (gx * g.Y + gy) * g.Z + gz;
    const bool in = !mask || mask[i];
    const WsCell c = ws_start(in, markers, f, negate, i);
    a.lam[i] = c.lam;
    b.lam[i] = c.lam;
    a.hop[i] = c.hop;
    b.hop[i] = c.hop;
    a.dst[i] = c.dst;
    b.dst[i] = c.dst;
    a.lab[i] = c.lab;
    b.lab[i] = c.lab;
    work |= in && !c.lab;
    mark |= c.lab != 0;
  }
  work = __syncthreads_or(work);
  mark = __syncthreads_or(mark);
  if (tid == 0) {
    brick_work[br] = work;
    brick_marker[br] = mark;
    if (work) flags[3] = 1;
  }
}

// One global pass: ws_core.hpp's relaxation, staged as in watershed.hip's ws_pass_kernel, on a
// brick with a one-voxel halo (20 B of state and a mask byte per voxel, 50 KB of LDS: three
// workgroups per CU).  A resident grid walks the bricks; a brick with nothing relaxable, or whose
// own and six face-adjacent bricks did not change in the previous pass, is skipped (a voxel reads
// only its six neighbours, so no other brick's change can reach it in one pass).  Brick flags
// rotate through three generations as the 2-D tile flags do.
__global__ __launch_bounds__(256) void ws3_pass_kernel(const double *__restrict__ f, int negate,
                                                       const int32_t *__restrict__ markers,
                                                       const uint8_t *__restrict__ mask, Vol g, WsState in,
                                                       WsState out, int32_t *__restrict__ changed,
                                                       const int32_t *__restrict__ prev_brick,
                                                       int32_t *__restrict__ cur_brick,
                                                       int32_t *__restrict__ next_brick,
                                                       const int32_t *__restrict__ brick_work, int nbx, int nby,
                                                       int nbz) {
  __shared__ double sl[HV];
  __shared__ int32_t sh[HV];
  __shared__ int32_t sd[HV];
  __shared__ int32_t sb[HV];
  __shared__ uint8_t sm[HV];
  const int tid = threadIdx.x;
  const int nbr = nbx * nby * nbz;
  for (int br = blockIdx.x; br < nbr; br += gridDim.x) {
    const Brick bk = brick_of(br, nby, nbz);
    const int bx = bk.bx, by = bk.by, bz = bk.bz;
    if (tid == 0) next_brick[br] = 0;
    if (!brick_work[br]) continue;
    {
      int act = prev_brick[br];
      if (bx > 0) act |= prev_brick[br - nby * nbz];
      if (bx + 1 < nbx) act |= prev_brick[br + nby * nbz];
      if (by > 0) act |= prev_brick[br - nbz];
      if (by + 1 < nby) act |= prev_brick[br + nbz];
      if (bz > 0) act |= prev_brick[br - 1];
      if (bz + 1 < nbz) act |= prev_brick[br + 1];
      if (!act) continue;
    }
    const int64_t x0 = bk.x0() - 1, y0 = bk.y0() - 1, z0 = bk.z0() - 1;
    __syncthreads();  // the previous brick's LDS is no longer read
    for_halo(tid, bk, g, [&](int idx, int64_t gx, int64_t gy, int64_t gz, bool inside) {
      if (inside) {
        const int64_t q = (gx * g.Y + gy) * g.Z + gz;
        const bool inm = !mask || mask[q];
        sl[idx] = in.lam[q];
        sh[idx] = in.hop[q];
        sd[idx] = in.dst[q];
        sb[idx] = in.lab[q];
        sm[idx] = (uint8_t)((inm ? 1 : 0) | ((inm && markers[q]) ? 2 : 0));
      } else {
        sl[idx] = __builtin_inf();
        sh[idx] = HOP_INF;
        sd[idx] = HOP_INF;
        sb[idx] = 0;
        sm[idx] = 0;
      }
    });
    __syncthreads();
    // thread tid owns the interior voxels (lx = k, ly = tid / 64, lz = tid % 64), k = 0..3; their
    // colour (lx + ly + lz) & 1 alternates with k
    int own[4];
    double fvk[4];
    const int ly = tid >> 6, lz = tid & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      own[k] = (k + 1) * SX + (ly + 1) * SY + (lz + 1) * SZ;
      const int64_t gx = x0 + 1 + k, gy = y0 + 1 + ly, gz = z0 + 1 + lz;
      const bool inside = gx < g.X && gy < g.Y && gz < g.Z;
      const double v = inside ? f[(gx * g.Y + gy) * g.Z + gz] : 0.0;
      fvk[k] = negate ? -v : v;
    }
    auto relax = [&](int i, double fv) -> bool {
      if ((sm[i] & 3) != 1) return false;  // outside the mask (or the volume), or a marker
      const int nb[6] = {i - SX, i - SY, i - SZ, i + SZ, i + SY, i + SX};
      WsCell best = ws_free();
#pragma unroll
      for (int d = 0; d < 6; ++d) {
        const int j = nb[d];
        const int32_t bj = sb[j];
        if (!bj || !(sm[j] & 1)) continue;
        const WsCell c{sl[j], sh[j], sd[j], bj};
        if (better(c, best)) best = c;
      }
      if (!best.lab) return false;
      const WsCell c = ws_step(best, fv);
      if (c.lab == sb[i] && c.lam == sl[i] && c.hop == sh[i] && c.dst == sd[i]) return false;
      sl[i] = c.lam;
      sh[i] = c.hop;
      sd[i] = c.dst;
      sb[i] = c.lab;
      return true;
    };
    bool any_change = false;
    const int par = (ly + lz) & 1;
    for (int it = 0; it < 4 * BV; ++it) {
      bool ch = false;
      // red-black: a voxel's six neighbours have the other colour, so one colour updates in place
      // from the other's current state (watershed.hip)
#pragma unroll
      for (int colour = 0; colour < 2; ++colour) {
        const int k0 = colour ^ par;  // this lane's voxels of the colour: k0, k0 + 2
        ch |= relax(k0 ? own[1] : own[0], k0 ? fvk[1] : fvk[0]);
        ch |= relax(k0 ? own[3] : own[2], k0 ? fvk[3] : fvk[2]);
        if (colour == 0) __syncthreads();  // red written before black reads it
      }
      any_change |= ch;
      if (!__syncthreads_or(ch)) break;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t gx = x0 + 1 + k, gy = y0 + 1 + ly, gz = z0 + 1 + lz;
      if (gx < g.X && gy < g.Y && gz < g.Z) {
        const int64_t q = (gx * g.Y + gy) * g.Z + gz;
        const int i = own[k];
        out.lam[q] = sl[i];
        out.hop[q] = sh[i];
        out.dst[q] = sd[i];
        out.lab[q] = sb[i];
      }
    }
    if (__syncthreads_or(any_change) && tid == 0) {
      *changed = 1;
      cur_brick[br] = 1;
    }
  }
}

// the voxels whose least-key reached in-mask neighbours carry different labels: only there can the
// heap's pop order decide a label
__global__ void ws3_contest_kernel(const int32_t *__restrict__ markers, const uint8_t *__restrict__ mask, Vol g,
                                   const double *__restrict__ lam, const int32_t *__restrict__ hop,
                                   const int32_t *__restrict__ lab, int32_t *__restrict__ count) {
  const int64_t n = g.n(), sy = g.Z, sx = g.Y * g.Z;
  int32_t c = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
    if ((mask && !mask[p]) || markers[p] || lam[p] == __builtin_inf()) continue;
    const int64_t z = p % g.Z, y = (p / g.Z) % g.Y, x = p / sx;
    const bool ok[6] = {x > 0, y > 0, z > 0, z + 1 < g.Z, y + 1 < g.Y, x + 1 < g.X};
    const int64_t nb[6] = {p - sx, p - sy, p - 1, p + 1, p + sy, p + sx};
    double bl = __builtin_inf();
    int32_t bh = HOP_INF, first = 0;
    bool diff = false;
    for (int d = 0; d < 6; ++d) {
      if (!ok[d]) continue;
      const int64_t q = nb[d];
      if (mask && !mask[q]) continue;
      const double lq = lam[q];
      if (lq == __builtin_inf()) continue;
      const int32_t hq = hop[q];
      if (lq < bl || (lq == bl && hq < bh)) {
        bl = lq;
        bh = hq;
        first = lab[q];
        diff = false;
      } else if (lq == bl && hq == bh) {
        diff |= lab[q] != first;
      }
    }
    c += diff;
  }
  c = hrf::wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

}  // namespace

extern "C" {

hrf_status hrf_cc_roots3(const void *img, int32_t dtype, int64_t X, int64_t Y, int64_t Z, int32_t conn,
                         int32_t *parent, hrf_stream_t stream) {
  HRF_TRY(check_vol(X, Y, Z, "cc_roots3"));
  HRF_REQUIRE(conn >= 1 && conn <= 3, "cc_roots3: connectivity must be 1 (6), 2 (18) or 3 (26)");
  HRF_REQUIRE(dtype == 0 || dtype == 1 || dtype == 2, "cc_roots3: dtype must be 0 (u8), 1 (i32) or 2 (u8 inverted)");
  if (X * Y * Z == 0) return HRF_OK;
  HRF_REQUIRE(img && parent, "cc_roots3: null buffer");
  const Vol g{X, Y, Z};
  if (dtype == 1) return run_cc3(LabelV{(const int32_t *)img}, g, conn, parent, (hipStream_t)stream);
  return run_cc3(MaskV{(const uint8_t *)img, dtype == 2}, g, conn, parent, (hipStream_t)stream);
}

hrf_status hrf_label3(const void *img, int32_t dtype, int64_t X, int64_t Y, int64_t Z, int32_t conn, int32_t *labels,
                      int32_t *parent_ws, int32_t *blk_ws, int32_t *nlab_dev, hrf_stream_t stream) {
  HRF_TRY(hrf_cc_roots3(img, dtype, X, Y, Z, conn, parent_ws, stream));
  return hrf_cc_number(parent_ws, X * Y * Z, labels, blk_ws, nlab_dev, stream);
}

hrf_status hrf_remove_small_objects_mask3(const uint8_t *mask, int64_t X, int64_t Y, int64_t Z, int64_t min_size,
                                          int32_t conn, uint8_t *out, int32_t *parent_ws, int32_t *size_ws,
                                          hrf_stream_t stream) {
  HRF_TRY(hrf_cc_roots3(mask, 0, X, Y, Z, conn, parent_ws, stream));
  const int64_t n = X * Y * Z;
  if (n == 0) return HRF_OK;
  HRF_REQUIRE(out && size_ws, "remove_small_objects_mask3: null buffer");
  HRF_TRY(hrf_cc_sizes(parent_ws, n, size_ws, stream));
  keep3_kernel<<<hrf::stream_grid(n), 256, 0, (hipStream_t)stream>>>(parent_ws, size_ws, n, min_size, out);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_fill_holes3(const uint8_t *mask, int64_t X, int64_t Y, int64_t Z, uint8_t *out, int32_t *parent_ws,
                           int32_t *flag_ws, hrf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  HRF_TRY(hrf_cc_roots3(mask, 2, X, Y, Z, 1, parent_ws, stream));  // background, 6-connected
  const int64_t n = X * Y * Z;
  if (n == 0) return HRF_OK;
  HRF_REQUIRE(out && flag_ws, "fill_holes3: null buffer");
  HRF_HIP(hipMemsetAsync(flag_ws, 0, sizeof(int32_t) * n, s));
  const Vol g{X, Y, Z};
  face_roots3_kernel<<<hrf::stream_grid(n), 256, 0, s>>>(parent_ws, g, flag_ws);
  fill3_finish_kernel<<<hrf::stream_grid(n), 256, 0, s>>>(mask, parent_ws, flag_ws, n, out);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_binary_erosion3(const uint8_t *mask, int64_t X, int64_t Y, int64_t Z, int32_t border_value,
                               uint8_t *out, hrf_stream_t stream) {
  HRF_TRY(check_vol(X, Y, Z, "binary_erosion3"));
  if (X * Y * Z == 0) return HRF_OK;
  HRF_REQUIRE(mask && out && mask != out, "binary_erosion3: bad buffers (in-place not supported)");
  morph3_kernel<true><<<hrf::stream_grid(X * Y * Z), 256, 0, (hipStream_t)stream>>>(mask, Vol{X, Y, Z},
                                                                                  border_value != 0, out);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_binary_dilation3(const uint8_t *mask, int64_t X, int64_t Y, int64_t Z, uint8_t *out,
                                hrf_stream_t stream) {
  HRF_TRY(check_vol(X, Y, Z, "binary_dilation3"));
  if (X * Y * Z == 0) return HRF_OK;
  HRF_REQUIRE(mask && out && mask != out, "binary_dilation3: bad buffers (in-place not supported)");
  morph3_kernel<false><<<hrf::stream_grid(X * Y * Z), 256, 0, (hipStream_t)stream>>>(mask, Vol{X, Y, Z}, 0, out);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_log10p1_f64(const double *x, int64_t n, double *out, hrf_stream_t stream) {
  HRF_REQUIRE(n >= 0, "log10p1: negative size");
  if (n == 0) return HRF_OK;
  HRF_REQUIRE(x && out, "log10p1: null buffer");
  log10p1_kernel<<<hrf::stream_grid(n), 256, 0, (hipStream_t)stream>>>(x, n, out);
  HRF_LAUNCHED();
  return HRF_OK;
}

// state: buffer a = lam, hop, dst (16 B per voxel; its labels are out_labels), buffer b = lam, hop,
// dst, lab (20 B), then per brick 3 generations of change flags, the work and the marker flags
int64_t hrf_watershed3_workspace_bytes(int64_t X, int64_t Y, int64_t Z) {
  if (check_vol(X, Y, Z, "watershed3_workspace_bytes")) return -1;
  const Vol g{X, Y, Z};
  return 36 * g.n() + 20 * g.bricks() + 256;
}

hrf_status hrf_watershed3_heap(const double *image, int32_t negate, const int32_t *markers, const uint8_t *mask,
                               int64_t X, int64_t Y, int64_t Z, int32_t *out_labels, hrf_stream_t stream) {
  HRF_TRY(check_vol(X, Y, Z, "watershed3_heap"));
  if (X * Y * Z == 0) return HRF_OK;
  HRF_REQUIRE(image && markers && out_labels, "watershed3_heap: null buffer");
  HRF_REQUIRE(out_labels != markers, "watershed3_heap: out_labels must not alias markers");
  return hrf::heap_flood3(image, negate, markers, mask, X, Y, Z, out_labels, (hipStream_t)stream);
}

hrf_status hrf_watershed3(const double *image, int32_t negate, const int32_t *markers, const uint8_t *mask, int64_t X,
                          int64_t Y, int64_t Z, int32_t *out_labels, void *state_ws, int32_t *flag_ws,
                          int32_t max_passes, int32_t *passes_host, int32_t *ties_host, hrf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  HRF_TRY(check_vol(X, Y, Z, "watershed3"));
  if (ties_host) ties_host[0] = ties_host[1] = ties_host[2] = 0;
  if (passes_host) *passes_host = 0;
  const Vol g{X, Y, Z};
  const int64_t n = g.n();
  if (n == 0) return HRF_OK;
  HRF_REQUIRE(image && markers && out_labels && state_ws && flag_ws, "watershed3: null buffer");
  HRF_REQUIRE(out_labels != markers, "watershed3: out_labels must not alias markers");
  const int64_t nbr = g.bricks();
  const int nbx = (int)g.bx(), nby = (int)g.by(), nbz = (int)g.bz();
  char *ws = (char *)state_ws;
  WsState a{(double *)ws, (int32_t *)(ws + 8 * n), out_labels, (int32_t *)(ws + 12 * n)};
  WsState b{(double *)(ws + 16 * n), (int32_t *)(ws + 24 * n), (int32_t *)(ws + 28 * n), (int32_t *)(ws + 32 * n)};
  int32_t *tf = (int32_t *)(ws + 36 * n);  // three generations of brick change flags
  int32_t *tw = tf + 3 * nbr, *tm = tw + nbr;
  int32_t hflag[4] = {0, 0, 0, 0};
  HRF_HIP(hipMemsetAsync(flag_ws, 0, sizeof(int32_t) * 4, s));
  ws3_init_kernel<<<(unsigned)nbr, 256, 0, s>>>(image, negate, markers, mask, g, nby, nbz, a, b, tw, tm, tf, flag_ws);
  HRF_LAUNCHED();
  HRF_HIP(hipMemcpyAsync(hflag, flag_ws, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, s));
  HRF_HIP(hipStreamSynchronize(s));
  // every in-mask voxel a marker (the reference's own call at :858): out_labels = markers x mask
  if (!hflag[3]) return HRF_OK;
  const unsigned pgrid = hrf::resident_grid(ws3_pass_kernel, 256, 0, nbr);
  int passes = 0;
  // batches of an even number of passes, one host read per batch (watershed.hip): the converged
  // state ends in buffer a, whose labels are out_labels
  for (int batch = 8;; batch = 4) {
    if (passes) HRF_HIP(hipMemsetAsync(flag_ws, 0, sizeof(int32_t) * 3, s));
    for (int k = 0; k < batch; ++k) {
      int32_t *cur = tf + (passes % 3) * nbr;
      const int32_t *prev = passes == 0 ? tm : tf + ((passes + 2) % 3) * nbr;
      int32_t *next = tf + ((passes + 1) % 3) * nbr;
      ws3_pass_kernel<<<pgrid, 256, 0, s>>>(image, negate, markers, mask, g, a, b, flag_ws + (k == batch - 1 ? 0 : 1),
                                            prev, cur, next, tw, nbx, nby, nbz);
      std::swap(a, b);
      ++passes;
    }
    HRF_LAUNCHED();
    ws3_contest_kernel<<<hrf::stream_grid(n), 256, 0, s>>>(markers, mask, g, a.lam, a.hop, a.lab, flag_ws + 2);
    HRF_LAUNCHED();
    HRF_HIP(hipMemcpyAsync(hflag, flag_ws, sizeof(int32_t) * 3, hipMemcpyDeviceToHost, s));
    HRF_HIP(hipStreamSynchronize(s));
    if (!hflag[0]) break;
    if (passes >= max_passes) {
      ::hrf::set_error("watershed3: not converged after %d passes (max_passes)", passes);
      return HRF_EINVAL;
    }
  }
  if (a.lab != out_labels) HRF_HIP(hipMemcpyAsync(out_labels, a.lab, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, s));
  const int32_t contested = hflag[2];
  if (contested > 0) HRF_TRY(hrf::heap_flood3(image, negate, markers, mask, X, Y, Z, out_labels, s));
  if (passes_host) *passes_host = passes;
  if (ties_host) {
    ties_host[0] = contested;
    ties_host[1] = contested > 0;
    ties_host[2] = passes;
  }
  return HRF_OK;
}

}  // extern "C"
