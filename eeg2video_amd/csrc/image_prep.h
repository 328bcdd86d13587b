// What the two preprocess kernels (vit.hip: image_prep_kernel, video.hip: video_prep_kernel) share: the view of the caller's frames
// and the byte a source sample stands for.
#pragma once
#include <hip/hip_runtime.h>

namespace e2v {
namespace {

struct PrepView {
    const void* p;
    long long s_n, s_img, s_c, s_y, s_x;         // clip, frame, channel, row, column -- in elements
};

__device__ __forceinline__ int prep_quantise(float x) {      // the bytes of frames_to_u8 on [0, 1]; NaN -> 0 (metrics.hip: quantise)
    x = x > 0.f ? x : 0.f;
    x = x < 1.f ? x : 1.f;
    return (int)(x * 255.f);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

template <bool F32>
__device__ __forceinline__ int prep_load(const PrepView& v, long long off) {
    return F32 ? prep_quantise(static_cast<const float*>(v.p)[off]) : (int)static_cast<const unsigned char*>(v.p)[off];
}

}  // namespace
}  // namespace e2v
