// Batched synthesis: the decode epilogue of KokoroEngine.generate_batch, where row b of a padded batch must get what the reference's
// B = 1 forward_inference gives utterance b alone.
//
//  row stop rule     the stop head / 30-frame energy rule / length bound of ONE row                     model/generator.py:67-88
//
// (The variance predictors of a ragged batch are the training path's own kernels with the row lengths as an argument: kk_im2col3_fwd,
// kk_groupnorm_relu_fwd and kk_rowdot_fwd with lens, kk_elem.hip / kk_norm.hip.)
#include "kk_common.h"
#include "kk_stop_rule.h"

namespace {

// ------------------------------------------------------------------ decode epilogue with the stop rule of each row
// One workgroup of 16 waves; wave w owns rows w, w + 16, ...  Everything a wave branches on (done flag, t, the row's bounds, its stop
// logit) is the same in all its lanes.  Filing the frame and the stop rule of a row: decode_row_file_and_stop (kk_stop_rule.h).
constexpr int EPI_WAVES = 16;

__global__ __launch_bounds__(64 * EPI_WAVES) void decode_epilogue_rows_kernel(
    const float *__restrict__ frame_out, const float *__restrict__ stop, float *__restrict__ mel_all, float *__restrict__ stop_all,
    int *__restrict__ t_dev, uint8_t *__restrict__ done, int *__restrict__ frames, int *__restrict__ live,
    const int *__restrict__ min_b, const int *__restrict__ expected_b, const int *__restrict__ max_b, int B, int L1, int M,
    float stop_threshold, float post_expected_stop_threshold) {
    const int t = *t_dev;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (t + 1 < L1) {
        for (int b = wave; b < B; b += EPI_WAVES) {
            if (done[b]) continue;
            const bool fin = decode_row_file_and_stop(frame_out, stop, mel_all, stop_all + (int64_t)t * B + b, min_b, expected_b, max_b,
                                                      b, t, lane, L1, M, stop_threshold, post_expected_stop_threshold);
            if (fin && lane == 0) {
                done[b] = 1;
                frames[b] = t + 1;
                atomicSub(live, 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *t_dev = t + 1;
}

}  // namespace

extern "C" int kk_decode_epilogue_rows(const float *frame_out, const float *stop, float *mel_all, float *stop_all, int *t_dev,
                                       uint8_t *done, int *frames, int *live, const int *min_b, const int *expected_b, const int *max_b,
                                       int B, int L1, int M, float stop_threshold, float post_expected_stop_threshold, void *stream) {
    KK_REQUIRE(frame_out && stop && mel_all && stop_all && t_dev && done && frames && live && min_b && expected_b && max_b && B > 0 &&
                   L1 > 1 && M > 0,
               "kk_decode_epilogue_rows: bad args");
    hipLaunchKernelGGL(decode_epilogue_rows_kernel, dim3(1), dim3(64 * EPI_WAVES), 0, (hipStream_t)stream, frame_out, stop, mel_all,
                       stop_all, t_dev, done, frames, live, min_b, expected_b, max_b, B, L1, M, stop_threshold,
                       post_expected_stop_threshold);
    KK_LAUNCH_CHECK("kk_decode_epilogue_rows");
    return 0;
}
