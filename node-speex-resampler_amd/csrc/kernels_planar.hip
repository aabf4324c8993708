// kernels_planar.hip -- channel planes <-> interleaved frames: the two passes either side of a planar call
// (engine.h, process_planar_device).  planar_gather transposes C planes of a stream into the interleaved image the FIR
// kernels read; planar_scatter transposes the image they wrote back into C planes.  Pure data movement.
//
// Grid = (frame tile, stream); the streams' arguments (PlanarPack) travel in the kernel-argument segment.  A tile is
// 256 lanes x 16 bytes of every plane: 1024 float frames, 2048 int16 frames.
//
// Vector path (C = 2, 4, 6, 8; whole tiles; plane base and plane stride multiples of 16 bytes -- decided per
// workgroup from the stream's arguments, so it is wave-uniform): lane t owns G = 16 / sizeof(T) consecutive frames.
//   gather:  C global loads of 16 B (one per plane: a wave reads 1 KiB of each plane), a register transpose into the C
//            16-byte chunks t*C .. t*C + C - 1 of the tile's interleaved image, written to LDS; then the image is read
//            back linearly, chunk it*256 + t, and stored: every global store is 16 B per lane, 4 KiB per workgroup.
//   scatter: the same steps backwards.
// The image lives in LDS in 16-byte chunks at swizzled positions (kSwizzle) such that both the strided access (lane
// stride C chunks) and the linear one are free of bank conflicts: ds_write_b128 is served in groups of 8 contiguous
// lanes over 32 banks (8 chunks), ds_read_b128 in four groups of 16 lanes over 64 banks (16 chunks).  The model of the
// two instructions in tests/test_cpu_planar.py checks every row of the table.
//
// Element path (any channel count, partial tiles, planes at any element-aligned address): 256 frames x up to 16
// channels at a time through an LDS image with an odd pitch, element by element; plane accesses run along the frames,
// interleaved accesses along the samples.
//
// The gather's image is read by the very next kernel and the scatter's source was written by the previous one: plain
// loads and stores throughout, so that the images can stay in L2 / Infinity Cache.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace speexhip {

SPEEXHIP_WARM_UNIT(planar)

namespace {

constexpr uint32_t kLanes = 256;
constexpr uint32_t kElemChannels = 16;             // channels per pass of the element path
constexpr uint32_t kElemPitch = kElemChannels + 1;  // ... and its LDS pitch (odd: conflict-free along the frames)

// chunk q of a tile's interleaved image lives at chunk q ^ ((q >> a) & m) ^ ((q >> b) & n) of the LDS image
struct Swizzle {
  uint32_t channels, scatter, a, m, b, n;
};
// clang-format off
constexpr Swizzle kSwizzle[] = {
    // C, scatter, a, m, b, n
    {2, 0, 1, 1, 3, 3}, {2, 1, 1, 1, 3, 3},
    {4, 0, 2, 1, 3, 7}, {4, 1, 2, 1, 3, 7},
    {6, 0, 3, 1, 3, 0}, {6, 1, 4, 1, 4, 0},
    {8, 0, 3, 7, 4, 7}, {8, 1, 3, 7, 4, 7},
};
// clang-format on
template <uint32_t C, bool kScatter>
__device__ __forceinline__ uint32_t swizzled(uint32_t q) {
  constexpr Swizzle z = kSwizzle[(C / 2 - 1) * 2 + (kScatter ? 1 : 0)];
  static_assert(z.channels == C && z.scatter == (kScatter ? 1u : 0u), "kSwizzle row order");
  return q ^ ((q >> z.a) & z.m) ^ ((q >> z.b) & z.n);
}

// Sample e (0 .. G*C-1, compile-time) of a lane's G frames, as held in registers: plane-major (r[c] = 16 bytes of
// plane c) or interleaved (o[k] = chunk k).
template <typename T>
__device__ __forceinline__ uint32_t sample_of(const uint4 &v, uint32_t i) {  // i-th T of 16 bytes, in the low bits
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if (sizeof(T) == 4) return w[i];
  return (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
}
template <typename T>
__device__ __forceinline__ uint4 pack_of(const uint32_t *e) {  // G samples -> 16 bytes
  if (sizeof(T) == 4) return make_uint4(e[0], e[1], e[2], e[3]);
  return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

template <typename T, uint32_t C, bool kScatter>
__device__ __forceinline__ void vector_tile(const PlanarStream &s, uint32_t tile0, uint4 *lds) {
  constexpr uint32_t G = 16 / sizeof(T);
  const uint32_t t = threadIdx.x;
  T *plane0 = static_cast<T *>(const_cast<void *>(s.planes)) + tile0 + t * G;
  uint4 *image = reinterpret_cast<uint4 *>(static_cast<T *>(s.inter) + static_cast<size_t>(tile0) * C);
  uint4 r[C], o[C];
  if (!kScatter) {
#pragma unroll
    for (uint32_t c = 0; c < C; c++) r[c] = *reinterpret_cast<const uint4 *>(plane0 + c * s.plane_stride);
#pragma unroll
    for (uint32_t k = 0; k < C; k++) {
      uint32_t e[G];
#pragma unroll
      for (uint32_t j = 0; j < G; j++) e[j] = sample_of<T>(r[(k * G + j) % C], (k * G + j) / C);
      lds[swizzled<C, false>(t * C + k)] = pack_of<T>(e);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t it = 0; it < C; it++) image[it * kLanes + t] = lds[swizzled<C, false>(it * kLanes + t)];
  } else {
#pragma unroll
    for (uint32_t it = 0; it < C; it++) lds[swizzled<C, true>(it * kLanes + t)] = image[it * kLanes + t];
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < C; k++) o[k] = lds[swizzled<C, true>(t * C + k)];
#pragma unroll
    for (uint32_t c = 0; c < C; c++) {
      uint32_t e[G];
#pragma unroll
      for (uint32_t g = 0; g < G; g++) e[g] = sample_of<T>(o[(g * C + c) / G], (g * C + c) % G);
      *reinterpret_cast<uint4 *>(plane0 + c * s.plane_stride) = pack_of<T>(e);
    }
  }
}

// frames [tile0, tile0 + n) of every channel, element by element
template <typename T, bool kScatter>
__device__ __forceinline__ void element_tile(const PlanarStream &s, uint32_t channels, uint32_t tile0, uint32_t n, T *lds) {
  const uint32_t t = threadIdx.x;
  T *planes = static_cast<T *>(const_cast<void *>(s.planes));
  T *image = static_cast<T *>(s.inter);
  for (uint32_t f0 = 0; f0 < n; f0 += kLanes) {
    const uint32_t nf = min(kLanes, n - f0);
    for (uint32_t c0 = 0; c0 < channels; c0 += kElemChannels) {
      const uint32_t cw = min(kElemChannels, channels - c0);
      T *first = image + (static_cast<size_t>(tile0) + f0) * channels + c0;  // sample (frame f0, channel c0) of the image
      if (!kScatter) {
        if (t < nf)
          for (uint32_t c = 0; c < cw; c++) lds[t * kElemPitch + c] = planes[(c0 + c) * s.plane_stride + tile0 + f0 + t];
        __syncthreads();
        for (uint32_t i = t; i < nf * cw; i += kLanes) {
          const uint32_t f = i / cw, c = i - f * cw;
          first[static_cast<size_t>(f) * channels + c] = lds[f * kElemPitch + c];
        }
      } else {
        for (uint32_t i = t; i < nf * cw; i += kLanes) {
          const uint32_t f = i / cw, c = i - f * cw;
          lds[f * kElemPitch + c] = first[static_cast<size_t>(f) * channels + c];
        }
        __syncthreads();
        if (t < nf)
          for (uint32_t c = 0; c < cw; c++) planes[(c0 + c) * s.plane_stride + tile0 + f0 + t] = lds[t * kElemPitch + c];
      }
      __syncthreads();
    }
  }
}

// C = 0: any channel count (element path only)
template <typename T, uint32_t C, bool kScatter>
__device__ __forceinline__ void transpose_tile(const PlanarPack &pack, uint32_t channels) {
  constexpr uint32_t kTile = kLanes * (16 / sizeof(T));
  constexpr uint32_t kVecBytes = C * kLanes * 16, kElemBytes = kLanes * kElemPitch * sizeof(T);
  __shared__ uint4 lds[(kVecBytes > kElemBytes ? kVecBytes : kElemBytes) / 16];
  const PlanarStream &s = pack.s[blockIdx.y];
  const uint32_t tile0 = blockIdx.x * kTile;
  if (s.planes == nullptr || tile0 >= s.frames) return;  // (silence, or a shorter stream of the launch)
  const uint32_t n = min(kTile, s.frames - tile0);
  if constexpr (C != 0) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(s.planes) | reinterpret_cast<uintptr_t>(s.inter) |
                           (s.plane_stride * sizeof(T))) & 15u) == 0;
    if (n == kTile && aligned) {
      vector_tile<T, C, kScatter>(s, tile0, lds);
      return;
    }
  }
  element_tile<T, kScatter>(s, channels, tile0, n, reinterpret_cast<T *>(lds));
}
template <typename T, uint32_t C>
__global__ __launch_bounds__(kLanes) void planar_gather(const PlanarPack pack, const uint32_t channels) {
  transpose_tile<T, C, false>(pack, channels);
}
template <typename T, uint32_t C>
__global__ __launch_bounds__(kLanes) void planar_scatter(const PlanarPack pack, const uint32_t channels) {
  transpose_tile<T, C, true>(pack, channels);
}

#define PLANAR_LAUNCH(C)                                                                            \
  if (kScatter)                                                                                     \
    hipLaunchKernelGGL((planar_scatter<T, C>), grid, block, 0, stream, pack, channels);             \
  else                                                                                              \
    hipLaunchKernelGGL((planar_gather<T, C>), grid, block, 0, stream, pack, channels);              \
  break
template <typename T, bool kScatter>
hipError_t launch_transpose(const PlanarPack &pack, uint32_t n, uint32_t channels, uint32_t max_frames, hipStream_t stream) {
  if (n == 0 || max_frames == 0 || channels == 0) return hipSuccess;
  const uint32_t tile = kLanes * (16 / sizeof(T));
  const dim3 grid((max_frames + tile - 1) / tile, n), block(kLanes);
  switch (channels) {
    case 2: PLANAR_LAUNCH(2);
    case 4: PLANAR_LAUNCH(4);
    case 6: PLANAR_LAUNCH(6);
    case 8: PLANAR_LAUNCH(8);
    default: PLANAR_LAUNCH(0);
  }
  return hipGetLastError();
}
#undef PLANAR_LAUNCH

}  // namespace

hipError_t launch_planar_gather(const PlanarPack &pack, uint32_t n, uint32_t channels, uint32_t max_frames, bool float_io,
                                hipStream_t stream) {
  return float_io ? launch_transpose<float, false>(pack, n, channels, max_frames, stream)
                  : launch_transpose<int16_t, false>(pack, n, channels, max_frames, stream);
}

hipError_t launch_planar_scatter(const PlanarPack &pack, uint32_t n, uint32_t channels, uint32_t max_frames, bool float_io,
                                 hipStream_t stream) {
  return float_io ? launch_transpose<float, true>(pack, n, channels, max_frames, stream)
                  : launch_transpose<int16_t, true>(pack, n, channels, max_frames, stream);
}

}  // namespace speexhip
