// vol.hpp -- the geometry of (X, Y, Z) volumes, row-major with Z fastest (voxel p = (x * Y + y) * Z
// + z), n = X*Y*Z < 2^31 - 2, and of the 4 x 4 x 64 brick (long in Z, the contiguous axis) that
// volume.hip and report3.hip stage in LDS, alone or with a one-voxel halo.
#pragma once
#include "common.hpp"

namespace hrf_vol {

constexpr int BX = 4, BY = 4, BZ = 64;                // brick: 1024 voxels, 256 threads x 4
constexpr int BV = BX * BY * BZ;
constexpr int HX = BX + 2, HY = BY + 2, HZ = BZ + 2;  // brick with its halo
constexpr int HV = HX * HY * HZ;
constexpr int SZ = 1, SY = HZ, SX = HY * HZ;          // halo-index strides

struct Vol {
  int64_t X, Y, Z;
  __host__ __device__ int64_t n() const { return X * Y * Z; }
  int64_t bx() const { return hrf::cdiv(X, BX); }
  int64_t by() const { return hrf::cdiv(Y, BY); }
  int64_t bz() const { return hrf::cdiv(Z, BZ); }
  int64_t bricks() const { return bx() * by() * bz(); }
};

inline hrf_status check_vol(int64_t X, int64_t Y, int64_t Z, const char *who) {
  HRF_REQUIRE(X >= 0 && Y >= 0 && Z >= 0, "%s: negative extent", who);
  // the product is formed only below the limit
  bool ok = true;
  if (X > 0 && Y > 0 && Z > 0) {
    constexpr int64_t lim = ((int64_t)1 << 31) - 2;
    ok = X < lim && Y < lim && X * Y < lim && Z < lim && (X * Y) <= (lim - 1) / Z;
  }
  HRF_REQUIRE(ok, "%s: volume too large (%lld x %lld x %lld, limit 2^31 - 2 voxels)", who, (long long)X, (long long)Y,
              (long long)Z);
  return HRF_OK;
}

// brick (bx, by, bz) of a grid of bricks and its first voxel
struct Brick {
  int bx, by, bz;
  __device__ __forceinline__ int64_t x0() const { return (int64_t)bx * BX; }
  __device__ __forceinline__ int64_t y0() const { return (int64_t)by * BY; }
  __device__ __forceinline__ int64_t z0() const { return (int64_t)bz * BZ; }
};
// brick br of an (nbx, nby, nbz) grid, Z fastest; I = the integer width br is divided in (the
// caller's: the watershed pass divides in 32 bits)
template <class I>
__device__ __forceinline__ Brick brick_of(I br, int nby, int nbz) {
  return Brick{(int)(br / ((I)nbz * nby)), (int)((br / nbz) % nby), (int)(br % nbz)};
}

// Every cell of the brick's halo, by a workgroup of HALO_THREADS (the launch bounds of the kernels
// that call it): fn(idx, gx, gy, gz, inside) with idx = hx * SX + hy * SY + hz the cell's halo
// index, (gx, gy, gz) its voxel and inside = within the volume.
constexpr int HALO_THREADS = 256;
template <class F>
__device__ __forceinline__ void for_halo(int tid, const Brick &b, const Vol &g, F fn) {
  const int64_t x0 = b.x0() - 1, y0 = b.y0() - 1, z0 = b.z0() - 1;
  for (int idx = tid; idx < HV; idx += HALO_THREADS) {
    const int hx = idx / SX, hy = (idx - hx * SX) / SY, hz = idx - hx * SX - hy * SY;
    const int64_t gx = x0 + hx, gy = y0 + hy, gz = z0 + hz;
    fn(idx, gx, gy, gz, gx >= 0 && gx < g.X && gy >= 0 && gy < g.Y && gz >= 0 && gz < g.Z);
  }
}

}  // namespace hrf_vol
