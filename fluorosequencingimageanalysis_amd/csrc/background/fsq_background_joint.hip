// fsq_background_joint.hip - np.mean of many ragged neighbour lists in one launch (include/fsq_background_joint.h): the
// interpolation of the background correction for joint signals of several colour channels, whose neighbourhoods have up to
// 3^8 - 1 = 6 560 entries.  One wavefront per list adds numpy's pairwise sum (stepfit/fsq_pairwise_wave.h).
//
// Bounds: a list is read only where its offsets ascend from >= 0, it is at most FSQ_BACKGROUND_JOINT_MAX_NEIGHBOURS long and
// d_nb is not null; an index read from it is used only where 0 <= index < n_counts; d_out[l] is written for l < n_lists alone.
#include <hip/hip_runtime.h>

#include "../fsq_common.h"
#include "../../../include/fsq_background_joint.h"
#include "../stepfit/fsq_pairwise_wave.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int MAX_NEIGHBOURS = FSQ_BACKGROUND_JOINT_MAX_NEIGHBOURS;
static_assert(MAX_NEIGHBOURS == PW_WAVE_MAX, "the wavefront's pairwise tree serves a whole neighbourhood");

__global__ void __launch_bounds__(THREADS) kbgj_means(const int32_t* nb, const int64_t* nb_off, long long n_lists, const double* count,
                                                      long long n_counts, double* out)
{
    const long long l = (long long)blockIdx.x * WAVES + threadIdx.x / WAVE;     // the wave's list
    if (l >= n_lists) return;
    const long long a = nb_off[l], b = nb_off[l + 1];
    double v = __builtin_nan("");
    if (a >= 0 && b >= a && b - a <= MAX_NEIGHBOURS && (nb != nullptr || b == a)) {
        const int32_t* list = nb + a;
        v = np_mean_wave([list, count, n_counts](int e) { const long long idx = list[e]; return idx >= 0 && idx < n_counts ? count[idx] : 0.0; },
                         (int)(b - a));
    }
    if (threadIdx.x % WAVE == 0) out[l] = v;
}

}  // namespace

extern "C" int fsq_background_neighbour_means(const int32_t* d_nb, const int64_t* d_nb_off, int64_t n_lists, const double* d_count,
                                              int64_t n_counts, double* d_out, void* stream_)
{
    if (n_lists < 0 || n_counts < 0 || n_lists > (int64_t)WAVES * 0x7fffffffll) return FSQ_EINVAL;
    if (n_lists == 0) return FSQ_OK;
    if (!d_nb_off || !d_out || (n_counts > 0 && !d_count)) return FSQ_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(kbgj_means, dim3((unsigned)((n_lists + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, d_nb, d_nb_off,
                       (long long)n_lists, d_count, (long long)n_counts, d_out);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
