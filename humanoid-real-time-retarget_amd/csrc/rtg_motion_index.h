// rtg_motion_index.h -- the index rule of the motion sampler (rtg_motion_sample.hip), host and device from one source:
// a query (clip, time) of a library of C clips -> the two frames it blends and the blend factor.  Plain C++ with no
// HIP header, so tests/motion_index_check.cpp compiles it with the host compiler alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTG_MIDX_FN __host__ __device__
#else
#define RTG_MIDX_FN
#endif

namespace rtg {

struct MotionIdx {
    int32_t i0, i1;   // frames of the clip, 0 <= i0 <= i1 <= len - 1, i1 - i0 <= 1
    float b;          // the blend factor, 0 <= b <= 1
    int32_t valid;    // 0 <= clip < C
};

// the query is valid iff 0 <= clip < C; an invalid one indexes nothing
RTG_MIDX_FN inline bool motion_clip_valid(int32_t clip, int32_t C) { return clip >= 0 && clip < C; }

// The phase p = (double)time * (double)fps, one f64 product; !(p > 0) -> 0 (NaN, -0, negatives).  p >= len - 1: the
// last frame, b = 0 (no wrap-around, and i1 never leaves the clip).  Otherwise i0 = trunc(p), i1 = i0 + 1 and
// b = (float)(p - (double)i0): the subtraction in f64, rounded to f32 once.
RTG_MIDX_FN inline MotionIdx motion_index(float time, float fps, int32_t len)
{
    double p = (double)time * (double)fps;
    if (!(p > 0.0)) p = 0.0;
    const int32_t last = len - 1;
    if (p >= (double)last) return MotionIdx{last, last, 0.0f, 1};
    const int32_t i0 = (int32_t)p;   // 0 <= p < len - 1 < 2^31: the conversion is defined
    return MotionIdx{i0, i0 + 1, (float)(p - (double)i0), 1};
}

}  // namespace rtg
