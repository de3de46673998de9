// report3.hip -- the per-cell report of a segmented (X, Y, Z) volume (biofilm_analysis.py:1359-1417,
// :280-289): per-label voxel moments and the regionprops fields the 3-D report reads, the label
// adjacency of skimage.future.graph.rag_boundary as a sparse set of edges, the barcode x barcode
// counts over that set, and the identification colour planes in Blender's voxel order.
// Volumes are vol.hpp's: row-major with Z fastest, n = X*Y*Z < 2^31 - 2.
//
// Moments follow stats.hip's moments_kernel: a wave holds 64 consecutive voxels, usually of one
// Z line; each distinct label of the wave leaves it as one set of four integer atomics, a run of
// equal labels along Z through closed forms.
//
// Edges: rag_boundary's edge set is, per voxel v, (min over the footprint, v) and (v, max over the
// footprint) where they differ from v (scipy's grey erosion / dilation with
// generate_binary_structure(3, conn); its reflect border repeats voxels of the in-volume window).
// A 4 x 4 x 64 brick is staged in LDS with a one-voxel halo (vol.hpp's brick and halo walk, as in
// volume.hip's watershed pass); an interior voxel (min == max == v) touches no global memory.  Keys
// (a << 32) | b, a < b, go into an open-addressing table: a probe reads with plain loads and only
// an empty slot is claimed by a 64-bit compare-and-swap, so the boundary voxels of one face, which
// mostly re-find their key, cost a load each.  A lane whose key equals its Z predecessor's leaves it
// to that lane.
//
// Planes: plane[ch][(z * Y + y) * X + x] = colour[label(x, y, z)][ch] is a transpose of every
// (X, Z) slab; a 64 x 64 tile of labels goes through LDS so that the label reads run along Z and
// the plane writes along X.
#include "rag_core.hpp"
#include "vol.hpp"
#include "wave.hpp"

namespace {

using namespace hrf_vol;

// ---- moments ------------------------------------------------------------------------------
// mom[l * 4 ..] = {count, sum x, sum y, sum z}, exact
__global__ void moments3_kernel(const int32_t *__restrict__ lab, int64_t Y, int64_t Z, int64_t n, int32_t maxlab,
                                unsigned long long *__restrict__ mom) {
  const int64_t n_up = (n + 63) / 64 * 64;
  const int lane = hrf::lane_id();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int32_t lnext = p < n ? lab[p] : 0;
  for (; p < n_up; p += stride) {
    const int32_t l = lnext;
    lnext = p + stride < n ? lab[p + stride] : 0;  // the next round's label is in flight during this one's atomics
    const bool ok = l > 0 && l <= maxlab;
    const int64_t line = p / Z, z = p - line * Z;
    const int64_t x = line / Y, y = line - x * Y;
    const int64_t key = ok ? (int64_t)l * 4 : 0;
    // the wave's 64 voxels on one Z line (always, when 64 divides Z): x and y are uniform, the count
    // is a popcount, and a label's lanes usually form one run [z0, z1] whose sum is a closed form
    const int64_t pb = p - lane, lb = pb / Z;
    const bool one_line = pb + 63 < n && (pb + 63) / Z == lb;
    unsigned long long pending = __ballot(ok);
    bool active = ok;
    while (pending) {
      const int leader = __ffsll((long long)pending) - 1;
      const int64_t k = __shfl(key, leader, 64);
      const bool m = active && key == k;
      const unsigned long long same = __ballot(m);
      unsigned long long a0, a1, a2, a3;
      if (one_line) {
        const unsigned long long cnt = (unsigned long long)__popcll(same);
        const unsigned long long xb = (unsigned long long)(lb / Y), yb = (unsigned long long)(lb - (lb / Y) * Y);
        const unsigned long long zb = (unsigned long long)(pb - lb * Z);
        const int hi = 63 - __builtin_clzll(same);
        a0 = cnt;
        a1 = cnt * xb;
        a2 = cnt * yb;
        if ((int)cnt == hi - leader + 1)
          a3 = (2 * zb + (unsigned long long)(leader + hi)) * cnt / 2;
        else
          a3 = hrf::wave_sum<unsigned long long>(m ? (unsigned long long)z : 0ull);
      } else {
        a0 = hrf::wave_sum<unsigned long long>(m ? 1ull : 0ull);
        a1 = hrf::wave_sum<unsigned long long>(m ? (unsigned long long)x : 0ull);
        a2 = hrf::wave_sum<unsigned long long>(m ? (unsigned long long)y : 0ull);
        a3 = hrf::wave_sum<unsigned long long>(m ? (unsigned long long)z : 0ull);
      }
      if (lane == leader) {
        atomicAdd(mom + k + 0, a0);
        atomicAdd(mom + k + 1, a1);
        atomicAdd(mom + k + 2, a2);
        atomicAdd(mom + k + 3, a3);
      }
      if (m) active = false;
      pending &= ~same;
    }
  }
}

// props[l * 5 ..] = {area, centroid x, y, z, valid}: the exact sums divided once by the count
__global__ void props3_kernel(const unsigned long long *__restrict__ mom, int32_t maxlab, double *__restrict__ props) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l > maxlab) return;
  const int64_t A = l ? (int64_t)mom[l * 4] : 0;
  double *o = props + l * 5;
  if (A <= 0) {
    o[0] = o[1] = o[2] = o[3] = o[4] = 0.0;
    return;
  }
  const double a = (double)A;
  o[0] = a;
  o[1] = (double)(int64_t)mom[l * 4 + 1] / a;
  o[2] = (double)(int64_t)mom[l * 4 + 2] / a;
  o[3] = (double)(int64_t)mom[l * 4 + 3] / a;
  o[4] = 1.0;
}

// ---- edges --------------------------------------------------------------------------------
constexpr unsigned long long EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// 1 when the key was new, 0 when it was present (or the table is full: *overflow = 1)
__device__ __forceinline__ int set_insert(unsigned long long *__restrict__ table, unsigned long long mask,
                                          unsigned long long key, int32_t *__restrict__ overflow) {
  unsigned long long slot = mix64(key) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
    unsigned long long cur = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return 0;
    if (cur == EMPTY) {
      cur = atomicCAS(table + slot, EMPTY, key);
      if (cur == EMPTY) return 1;
      if (cur == key) return 0;
    }
  }
  *overflow = 1;
  return 0;
}

template <int CONN>
__global__ __launch_bounds__(256) void rag_edges3_kernel(const int32_t *__restrict__ lab, int64_t X, int64_t Y,
                                                         int64_t Z, int nbx, int nby, int nbz,
                                                         unsigned long long *__restrict__ table,
                                                         unsigned long long mask, int32_t *__restrict__ info) {
  __shared__ int32_t sv[HV];
  const int tid = threadIdx.x, lane = hrf::lane_id();
  const int64_t nbr = (int64_t)nbx * nby * nbz;
  int inserted = 0;
  for (int64_t br = blockIdx.x; br < nbr; br += gridDim.x) {
    const Brick bk = brick_of(br, nby, nbz);
    const int64_t x0 = bk.x0() - 1, y0 = bk.y0() - 1, z0 = bk.z0() - 1;
    __syncthreads();  // the previous brick's LDS is no longer read
    // a halo voxel outside the volume repeats the nearest voxel inside it: for a voxel v and an
    // offset d of its footprint, clamp(v + d) = v + d' with d' the offset d less its components
    // that leave the volume, which is again in the footprint (it has no more non-zero components)
    for_halo(tid, bk, Vol{X, Y, Z}, [&](int idx, int64_t gx, int64_t gy, int64_t gz, bool) {
      gx = gx < 0 ? 0 : (gx >= X ? X - 1 : gx);
      gy = gy < 0 ? 0 : (gy >= Y ? Y - 1 : gy);
      gz = gz < 0 ? 0 : (gz >= Z ? Z - 1 : gz);
      sv[idx] = lab[(gx * Y + gy) * Z + gz];
    });
    __syncthreads();
    // thread tid owns the voxels (lx = k, ly = tid / 64, lz = tid % 64), k = 0..3
    const int ly = tid >> 6, lz = tid & 63;
    unsigned long long last_lo = EMPTY, last_hi = EMPTY;
#pragma unroll
    for (int k = 0; k < BX; ++k) {
      const int i = (k + 1) * SX + (ly + 1) * SY + (lz + 1) * SZ;
      const bool inside = x0 + 1 + k < X && y0 + 1 + ly < Y && z0 + 1 + lz < Z;
      const int32_t v = sv[i];
      int32_t mn = v, mx = v;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dz = -1; dz <= 1; ++dz) {
            if ((dx != 0) + (dy != 0) + (dz != 0) > CONN || (dx == 0 && dy == 0 && dz == 0)) continue;
            const int32_t u = sv[i + dx * SX + dy * SY + dz * SZ];
            mn = u < mn ? u : mn;
            mx = u > mx ? u : mx;
          }
      // (mn, v) needs 0 <= mn (then v > mn >= 0), (v, mx) needs 0 <= v
      unsigned long long klo = EMPTY, khi = EMPTY;
      if (inside && mn != v && mn >= 0) klo = ((unsigned long long)(uint32_t)mn << 32) | (uint32_t)v;
      if (inside && mx != v && v >= 0) khi = ((unsigned long long)(uint32_t)v << 32) | (uint32_t)mx;
      // a key equal to the Z predecessor's (the lane below) or to this thread's previous voxel's is
      // theirs to insert
      const unsigned long long plo = __shfl_up(klo, 1, 64), phi = __shfl_up(khi, 1, 64);
      const bool dlo = klo != EMPTY && !(lane > 0 && plo == klo) && klo != last_lo;
      const bool dhi = khi != EMPTY && !(lane > 0 && phi == khi) && khi != last_hi;
      if (dlo) inserted += set_insert(table, mask, klo, info + 1);
      if (dhi) inserted += set_insert(table, mask, khi, info + 1);
      last_lo = klo;
      last_hi = khi;
    }
  }
  inserted = hrf::wave_sum<int>(inserted);
  if (lane == 0 && inserted) atomicAdd(info, inserted);
}

// the edges' counts (rag_core.hpp) over a list of keys
__global__ void adjacency_edges_kernel(const int64_t *__restrict__ keys, int64_t E, const int32_t *__restrict__ bc,
                                       const uint8_t *__restrict__ keep, int64_t maxlab, int32_t R,
                                       unsigned long long *__restrict__ adj, unsigned long long *__restrict__ adjf) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = (unsigned long long)keys[e];
    const int64_t a = (int64_t)(key >> 32), b = (int64_t)(key & 0xffffffffull);
    if (b <= maxlab) hrf::count_edge(a, b, bc, keep, R, adj, adjf);
  }
}

// ---- planes -------------------------------------------------------------------------------
constexpr int TP = 64;  // tile edge on X and on Z

__global__ __launch_bounds__(256) void paint_planes3_kernel(const int32_t *__restrict__ lab, int64_t X, int64_t Y,
                                                            int64_t Z, const float *__restrict__ colour,
                                                            int32_t ncell, float *__restrict__ planes, int64_t ntx,
                                                            int64_t ntz) {
  __shared__ int32_t tile[TP][TP + 1];
  const int64_t n = X * Y * Z;
  const int64_t ntile = ntx * Y * ntz;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t tz = t % ntz, y = (t / ntz) % Y, tx = t / (ntz * Y);
    const int64_t xb = tx * TP, zb = tz * TP;
    __syncthreads();
    for (int r = w; r < TP; r += 4) {  // a row of the tile: one x, 64 consecutive z
      const int64_t x = xb + r, z = zb + lane;
      int32_t l = 0;
      if (x < X && z < Z) l = lab[(x * Y + y) * Z + z];
      tile[r][lane] = (l < 0 || l > ncell) ? 0 : l;
    }
    __syncthreads();
    for (int r = w; r < TP; r += 4) {  // a column of the tile: one z, 64 consecutive x
      const int64_t z = zb + r, x = xb + lane;
      if (z >= Z || x >= X) continue;
      const int64_t l3 = (int64_t)tile[lane][r] * 3;
      const int64_t q = (z * Y + y) * X + x;
      planes[q] = colour[l3];
      planes[n + q] = colour[l3 + 1];
      planes[2 * n + q] = colour[l3 + 2];
    }
  }
}

}  // namespace

extern "C" {

hrf_status hrf_region_moments3(const int32_t *labels, int64_t X, int64_t Y, int64_t Z, int32_t maxlab, int64_t *mom,
                               hrf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  HRF_REQUIRE(maxlab >= 0 && mom, "region_moments3: bad arguments");
  HRF_TRY(check_vol(X, Y, Z, "region_moments3"));
  HRF_HIP(hipMemsetAsync(mom, 0, sizeof(int64_t) * 4 * ((size_t)maxlab + 1), s));
  const int64_t n = X * Y * Z;
  if (n == 0) return HRF_OK;
  HRF_REQUIRE(labels, "region_moments3: null labels");
  // every resident slot: a thread's rounds are serial (load, ballots, atomics), so the pass is as
  // fast as there are waves in flight
  const unsigned grid = hrf::resident_grid(moments3_kernel, 256, 0, hrf::cdiv(n, 256));
  moments3_kernel<<<grid, 256, 0, s>>>(labels, Y, Z, n, maxlab, (unsigned long long *)mom);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_region_props3(const int64_t *mom, int32_t maxlab, double *props, hrf_stream_t stream) {
  HRF_REQUIRE(maxlab >= 0 && mom && props, "region_props3: bad arguments");
  props3_kernel<<<(unsigned)hrf::cdiv((int64_t)maxlab + 1, 256), 256, 0, (hipStream_t)stream>>>(
      (const unsigned long long *)mom, maxlab, props);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_rag_edges3(const int32_t *labels, int64_t X, int64_t Y, int64_t Z, int32_t conn, uint64_t *table,
                          int64_t cap, int32_t *info_dev, hrf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  HRF_REQUIRE(conn >= 1 && conn <= 3, "rag_edges3: conn must be 1, 2 or 3");
  HRF_REQUIRE(table && info_dev && cap >= 2 && cap <= ((int64_t)1 << 40) && (cap & (cap - 1)) == 0,
              "rag_edges3: the capacity must be a power of two >= 2");
  HRF_TRY(check_vol(X, Y, Z, "rag_edges3"));
  HRF_HIP(hipMemsetAsync(table, 0xff, sizeof(uint64_t) * (size_t)cap, s));
  HRF_HIP(hipMemsetAsync(info_dev, 0, 2 * sizeof(int32_t), s));
  if (X * Y * Z == 0) return HRF_OK;
  HRF_REQUIRE(labels, "rag_edges3: null labels");
  const int64_t nbx = hrf::cdiv(X, BX), nby = hrf::cdiv(Y, BY), nbz = hrf::cdiv(Z, BZ);
  const int64_t nbr = nbx * nby * nbz;
  unsigned long long *t = (unsigned long long *)table;
  const unsigned long long mask = (unsigned long long)cap - 1;
  if (conn == 1)
    rag_edges3_kernel<1><<<hrf::resident_grid(rag_edges3_kernel<1>, 256, 0, nbr), 256, 0, s>>>(
        labels, X, Y, Z, (int)nbx, (int)nby, (int)nbz, t, mask, info_dev);
  else if (conn == 2)
    rag_edges3_kernel<2><<<hrf::resident_grid(rag_edges3_kernel<2>, 256, 0, nbr), 256, 0, s>>>(
        labels, X, Y, Z, (int)nbx, (int)nby, (int)nbz, t, mask, info_dev);
  else
    rag_edges3_kernel<3><<<hrf::resident_grid(rag_edges3_kernel<3>, 256, 0, nbr), 256, 0, s>>>(
        labels, X, Y, Z, (int)nbx, (int)nby, (int)nbz, t, mask, info_dev);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_barcode_adjacency_edges(const int64_t *keys, int64_t E, const int32_t *bc_of_label,
                                       const uint8_t *keep_of_label, int32_t maxlab, int32_t R, int64_t *adj,
                                       int64_t *adj_filtered, hrf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  HRF_REQUIRE(maxlab >= 0 && R >= 1 && E >= 0 && bc_of_label && adj, "barcode_adjacency_edges: bad arguments");
  HRF_REQUIRE(!adj_filtered || keep_of_label, "barcode_adjacency_edges: a filtered matrix needs keep flags");
  HRF_HIP(hipMemsetAsync(adj, 0, sizeof(int64_t) * (size_t)R * R, s));
  if (adj_filtered) HRF_HIP(hipMemsetAsync(adj_filtered, 0, sizeof(int64_t) * (size_t)R * R, s));
  if (E == 0) return HRF_OK;
  HRF_REQUIRE(keys, "barcode_adjacency_edges: null keys");
  adjacency_edges_kernel<<<hrf::stream_grid(E), 256, 0, s>>>(keys, E, bc_of_label, keep_of_label, maxlab, R,
                                                             (unsigned long long *)adj,
                                                             (unsigned long long *)adj_filtered);
  HRF_LAUNCHED();
  return HRF_OK;
}

hrf_status hrf_paint_planes3(const int32_t *labels, int64_t X, int64_t Y, int64_t Z, const float *colour,
                             int32_t ncell, float *planes, hrf_stream_t stream) {
  HRF_REQUIRE(ncell >= 0 && colour, "paint_planes3: bad arguments");
  HRF_TRY(check_vol(X, Y, Z, "paint_planes3"));
  if (X * Y * Z == 0) return HRF_OK;
  HRF_REQUIRE(labels && planes, "paint_planes3: null buffer");
  const int64_t ntx = hrf::cdiv(X, TP), ntz = hrf::cdiv(Z, TP);
  const int64_t ntile = ntx * Y * ntz;
  const unsigned grid = (unsigned)(ntile < (int64_t)1 << 20 ? ntile : (int64_t)1 << 20);
  paint_planes3_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(labels, X, Y, Z, colour, ncell, planes, ntx, ntz);
  HRF_LAUNCHED();
  return HRF_OK;
}

}  // extern "C"
