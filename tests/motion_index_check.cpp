// motion_index_check.cpp -- the motion sampler's index rule (csrc/rtg_motion_index.h, the function the kernel calls)
// run on the host over the time families x clip lengths x frame rates x clip ids, with its invariants asserted:
// 0 <= i0 <= i1 <= L - 1, i1 - i0 <= 1, 0 <= b <= 1, invalid clip ids flagged.  Prints one line per case,
//   L fps_bits time_bits clip C valid i0 i1 b_bits
// which tests/test_motion_sample_host.py compares with the numpy restatement of the rule, and "N cases, M failures".
// Host C++ only: built by the test with g++, and once more with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rtg_motion_index.h"

static uint32_t bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

int main()
{
    const int lengths[] = {1, 2, 3, 17, 130};
    const float rates[] = {1.0f, 30.0f, 120.0f, 1e-3f, 3e38f};
    const int C = 5;
    const int32_t clips[] = {-1, 0, C - 1, C, INT32_MIN, INT32_MAX};
    const float inf = std::numeric_limits<float>::infinity();
    long cases = 0, failures = 0;
    for (const int L : lengths) {
        for (const float fps : rates) {
            std::vector<float> times;
            for (int k = 0; k < L; ++k) {   // the frame instants and one ulp either side
                const float t = (float)((double)k / (double)fps);
                times.push_back(t);
                times.push_back(std::nextafter(t, inf));
                times.push_back(std::nextafter(t, -inf));
                times.push_back((float)(((double)k + 0.37) / (double)fps));
            }
            const float edge[] = {0.0f, -0.0f, -1.0f, -1e-30f, 1e-45f, -1e-45f, (float)((double)(L - 1) / (double)fps),
                                  (float)((double)L / (double)fps), (float)(((double)L + 100.5) / (double)fps), 3e38f,
                                  inf, -inf, std::numeric_limits<float>::quiet_NaN(),
                                  1.00000011920928955078125f /* 1 + 2^-23 */};
            for (const float t : edge) times.push_back(t);
            for (const float t : times) {
                for (const int32_t clip : clips) {
                    const bool valid = rtg::motion_clip_valid(clip, C);
                    ++cases;
                    if (valid != (clip >= 0 && clip < C)) ++failures;
                    if (!valid) {   // an invalid query indexes nothing: the kernel never runs the rule on its clip
                        printf("%d %u %u %d %d 0 0 0 0\n", L, bits(fps), bits(t), clip, C);
                        continue;
                    }
                    const rtg::MotionIdx ix = rtg::motion_index(t, fps, L);
                    const bool ok = 0 <= ix.i0 && ix.i0 <= ix.i1 && ix.i1 <= L - 1 && ix.i1 - ix.i0 <= 1 &&
                                    ix.b >= 0.0f && ix.b <= 1.0f && ix.valid == 1;
                    if (!ok) {
                        ++failures;
                        fprintf(stderr, "FAIL L=%d fps=%g t=%g: i0=%d i1=%d b=%g\n", L, (double)fps, (double)t, ix.i0,
                                ix.i1, (double)ix.b);
                    }
                    printf("%d %u %u %d %d 1 %d %d %u\n", L, bits(fps), bits(t), clip, C, ix.i0, ix.i1, bits(ix.b));
                }
            }
        }
    }
    {   // a blend factor that rounds up to 1.0f: (1 + 2^-23) (1 - 2^-23) = 1 - 2^-46
        const rtg::MotionIdx ix = rtg::motion_index(1.00000011920928955078125f, 0.99999988079071044921875f, 3);
        ++cases;
        if (!(ix.i0 == 0 && ix.i1 == 1 && ix.b == 1.0f)) ++failures;
    }
    printf("%ld cases, %ld failures\n", cases, failures);
    return failures ? 1 : 0;
}
