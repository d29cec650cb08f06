// The stop rule of ONE row of a batched decode (model/generator.py:67-88), shared by the two decode epilogues: kk_synth.hip
// (decode_epilogue_rows_kernel, every row at the same frame t) and kk_stream.hip (decode_epilogue_slots_kernel, slot b at its own t).
#pragma once
#include "kk_common.h"

namespace {

// Called by one whole wave for row b at frame t (0 <= t < L1 - 1; what it branches on is the same in all lanes): files frame_out[b]
// under row t + 1 of the row's mel_all [L1][M] and the stop logit in *stop_slot (the caller's layout), and returns whether the row
// ends with this frame: its length bound, the stop head above the threshold of its side of `expected`, or the last 30 frames (rows
// t-28 .. t of earlier launches + this one) quiet in the mean, summed in fp64: lanes stride the frame, then the 29, then wave_sum_d.
__device__ __forceinline__ bool decode_row_file_and_stop(
    const float *__restrict__ frame_out, const float *__restrict__ stop, float *__restrict__ mel_all, float *__restrict__ stop_slot,
    const int *__restrict__ min_b, const int *__restrict__ expected_b, const int *__restrict__ max_b, int b, int t, int lane, int L1,
    int M, float stop_threshold, float post_expected_stop_threshold) {
    const float *fo = frame_out + (int64_t)b * M;
    float *mrow = mel_all + (int64_t)b * L1 * M;
    double s = 0.0;
    for (int c = lane; c < M; c += 64) {
        const float v = fo[c];
        mrow[(int64_t)(t + 1) * M + c] = v;
        s += (double)v;
    }
    const float logit = stop[b];
    if (lane == 0) *stop_slot = logit;
    bool fin = t + 1 >= max_b[b];
    if (!fin && t >= min_b[b]) {
        const float thr = t < expected_b[b] ? stop_threshold : fminf(stop_threshold, post_expected_stop_threshold);
        const float prob = 1.f / (1.f + expf(-logit));
        if (prob > thr) {
            fin = true;
        } else if (t + 1 >= 30) {
            const float *tail = mrow + (int64_t)(t - 28) * M;             // 29 earlier frames, contiguous
            for (int i = lane; i < 29 * M; i += 64) s += (double)tail[i];
            s = wave_sum_d(s);
            fin = s / (30.0 * M) < -9.5;
        }
    }
    return fin;
}

}  // namespace
