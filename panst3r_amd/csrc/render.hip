// A z-buffered point splatter: the panoptic cloud (csrc/cloud.hip) or its voxel fusion (csrc/voxel.hip) seen from any pinhole camera -> per pixel the
// nearest point's row, depth, panoptic id and colours.  The reference has no such stage (its demo hands the cloud to an interactive viewer); restated
// in tests/render_ref.py, [restated, parity unpinned].  Two kernels around a uint64 [B, H, W] buffer the caller clears to all ones:
//   splat    one thread per (point, camera), the camera on grid.y: world -> camera, cull, project, then a 64-bit atomicMin of
//            key = (bits(zc) << 32) | row into every pixel of the point's (2r + 1)^2 footprint, clipped to the image.  zc > 0, so its bit pattern
//            orders as an unsigned integer: the smallest key is the nearest point, equal depths go to the smallest row.
//   resolve  one thread per pixel: the winner's row and depth out of the key, pan / rgb / colors gathered from that row, plain vector stores.
// The arithmetic is part of the contract (include/panst3r_hip.h): contraction is off for the whole file, every fp32 product and sum is rounded on
// its own, and the perspective quotient is taken in fp64 and rounded once (affine34 and project of pinhole.h).  INTEGER atomics only: the buffer's final state is the minimum
// over a fixed set of keys, whatever the schedule - two calls return identical bytes.
// `precheck`: the buffer has far fewer cells than the cloud has points (9.8 M points on 0.2 M pixels at the benchmark's scene size), so most
// candidates lose.  A relaxed device-scope load of the cell first, and the atomic only for a key that is smaller than what the load saw, trades
// most of the atomics for L2 reads; a stale read can only let a losing atomic through, never suppress a winning one (the cell only decreases).
// What bounds the kernels: splat reads 12 bytes per (point, camera) - 118 MB per camera at 9.8 M points, tens of microseconds of HBM time - and
// issues up to (2r + 1)^2 8-byte read-modify-writes per point that are served by the L2 / memory side one 64-byte request per few lanes, so the
// expectation is that atomics and L2 bound it, not HBM (the measured times and the A/B of the pre-check are in docs/experiments.md).  resolve is a
// coalesced read of the buffer plus scattered 28-byte gathers and 44 bytes of stores per pixel: bound by the gathers' latency, small next to splat.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "pinhole.h"             // affine34, project, PH_CAM; and through it wave_ops.h: rn_mul, rn_div

#pragma clang fp contract(off)

namespace pst {

constexpr int RD_T = 256;
constexpr unsigned long long RD_EMPTY = ~0ull;                     // no key is all ones: bits(zc) = 0xFFFFFFFF is a NaN, and a NaN is culled
constexpr float RD_LIM = 1048576.f;                                // |u|, |v| <= 2^20: px +- r and py +- r cannot overflow

template <bool PRECHECK>
__global__ __launch_bounds__(RD_T) void render_splat_kernel(const float* __restrict__ points, int64_t M, const float* __restrict__ cams, int H, int W,
                                                            float half_size, int radius, int max_radius, unsigned long long* __restrict__ zbuf) {
  const int64_t i = (int64_t)blockIdx.x * RD_T + threadIdx.x;
  if (i >= M) return;
  const float* __restrict__ c = cams + (int64_t)blockIdx.y * PH_CAM;              // uniform: scalar loads
  const float P[3] = {points[i * 3 + 0], points[i * 3 + 1], points[i * 3 + 2]};
  float pc[3], u, v;
  affine34(c, P, pc);
  const float f = c[12], cx = c[13], cy = c[14], near = c[15], zc = pc[2];
  if (!(fabsf(pc[0]) <= PST_FMAX && fabsf(pc[1]) <= PST_FMAX && fabsf(zc) <= PST_FMAX) || !(zc >= near)) return;      // finite3, written out: pinhole.h says why
  if (!project(f, f, cx, cy, pc, RD_LIM, u, v)) return;
  const int px = (int)floorf(u), py = (int)floorf(v);
  // r = min(max_radius, max(radius, floor(f half_size / zc))): the quotient is >= 0 (or +inf), clamped as a float before it becomes an int
  const int rs = (int)fminf(floorf(rn_div(rn_mul(f, half_size), zc)), (float)max_radius);
  const int r = min(max_radius, max(radius, rs));
  const int x0 = max(px - r, 0), x1 = min(px + r, W - 1), y0 = max(py - r, 0), y1 = min(py + r, H - 1);                // |px|, |py| <= 2^20: no overflow
  if (x0 > x1 || y0 > y1) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(zc) << 32) | (unsigned long long)(uint32_t)i;
  unsigned long long* __restrict__ zb = zbuf + (int64_t)blockIdx.y * H * W;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {                             // 0 <= yy < H, 0 <= xx < W: inside the camera's H x W cells
      unsigned long long* p = zb + (int64_t)yy * W + xx;
      if constexpr (PRECHECK)
        if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;
      atomicMin(p, key);
    }
}

__global__ __launch_bounds__(RD_T) void render_resolve_kernel(const unsigned long long* __restrict__ zbuf, int64_t npix, int64_t M, const float* __restrict__ rgb,
                                                              const float* __restrict__ colors, const int32_t* __restrict__ pan, int64_t* __restrict__ index,
                                                              float* __restrict__ depth, int32_t* __restrict__ out_pan, float* __restrict__ out_rgb,
                                                              float* __restrict__ out_colors) {
  const int64_t p = (int64_t)blockIdx.x * RD_T + threadIdx.x;
  if (p >= npix) return;
  const unsigned long long key = zbuf[p];
  const int64_t row = (int64_t)(uint32_t)key;
  const bool hit = key != RD_EMPTY && row < M;                      // (row < M always holds for a buffer that splat filled: no read outside the cloud)
  index[p] = hit ? row : -1;
  depth[p] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
  out_pan[p] = hit ? pan[row] : 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out_rgb[p * 3 + a] = hit ? rgb[row * 3 + a] : 0.f;
    out_colors[p * 3 + a] = hit ? colors[row * 3 + a] : 0.f;
  }
}

}  // namespace pst

extern "C" int pst_render_max_radius(void) { return PST_RENDER_MAX_RADIUS; }

extern "C" int pst_render_splat(const float* points, int64_t M, const float* cams, int ncams, int H, int W, float half_size, int radius, int max_radius,
                                uint64_t* zbuf, int precheck, void* stream) {
  using namespace pst;
  if (M <= 0 || M > 0xffffffffLL || ncams < 1 || ncams > 65535 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffffLL / ncams) {
    set_error("render_splat: bad shape (M=%lld in [1, 2^32 - 1], %d cameras in [1, 65535], %d x %d pixels, cameras x pixels < 2^31)", (long long)M, ncams, H, W);
    return PST_EINVAL;
  }
  if (radius < 0 || radius > PST_RENDER_MAX_RADIUS || max_radius < 0 || max_radius > PST_RENDER_MAX_RADIUS || !(half_size >= 0.f) || !(half_size <= PST_FMAX)) {
    set_error("render_splat: radius=%d / max_radius=%d outside [0, %d] or half_size=%g not a finite number >= 0", radius, max_radius, PST_RENDER_MAX_RADIUS,
              (double)half_size);
    return PST_EINVAL;
  }
  if (!points || !cams || !zbuf) { set_error("render_splat: null operand"); return PST_EINVAL; }
  const dim3 grid(blocks_for(M, RD_T).x, (unsigned)ncams);
  if (precheck) hipLaunchKernelGGL(render_splat_kernel<true>, grid, dim3(RD_T), 0, (hipStream_t)stream, points, M, cams, H, W, half_size, radius, max_radius,
                                   (unsigned long long*)zbuf);
  else hipLaunchKernelGGL(render_splat_kernel<false>, grid, dim3(RD_T), 0, (hipStream_t)stream, points, M, cams, H, W, half_size, radius, max_radius,
                          (unsigned long long*)zbuf);
  return check_launch("render_splat");
}

extern "C" int pst_render_resolve(const uint64_t* zbuf, int64_t npix, int64_t M, const float* rgb, const float* colors, const int32_t* pan, int64_t* index,
                                  float* depth, int32_t* out_pan, float* out_rgb, float* out_colors, void* stream) {
  using namespace pst;
  if (npix <= 0 || npix > 0x7fffffffLL || M <= 0 || M > 0xffffffffLL) {
    set_error("render_resolve: bad shape (%lld pixels in [1, 2^31 - 1], M=%lld in [1, 2^32 - 1])", (long long)npix, (long long)M); return PST_EINVAL;
  }
  if (!zbuf || !rgb || !colors || !pan || !index || !depth || !out_pan || !out_rgb || !out_colors) { set_error("render_resolve: null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(render_resolve_kernel, blocks_for(npix, RD_T), dim3(RD_T), 0, (hipStream_t)stream, (const unsigned long long*)zbuf, npix, M,
                     rgb, colors, pan, index, depth, out_pan, out_rgb, out_colors);
  return check_launch("render_resolve");
}
