// fsq_experiment.hip - the glue between the stages of a sequence experiment (include/fsq_experiment.h), gfx950.
//
//   kx_scan        one block: exclusive scan of max(x, 0) over an int32 array (peaks per frame -> first record of every frame,
//                  Spots per frame -> first Spot of every frame, traces per sequence -> first row of every sequence)
//   kx_accept      one block per frame, one lane per record: Spot.__init__'s acceptance test (flexlibrary.py:98-121) on the
//                  record's key and fitted centre; the key and the verdict go to the workspace, the block counts its Spots
//   kx_compact     one block per frame: ordered compaction of the accepted keys (ballot + prefix per wave, wave totals through
//                  LDS, chunks of the frame in order) - record order is the contract, so no atomics
//   kx_trace_rows  one lane per (trace, frame): the spot number of fsq_greedy_tracking's trace row -> (h, w) and table row
// Nothing here does arithmetic beyond comparisons: both entries are bound by memory traffic.  kx_accept touches 24 of a
// record's 378 / 428 bytes (two or three 128-byte lines per record, the stride being no multiple of a line), kx_compact moves
// 9 + 12 bytes per record through the workspace.  A record's fields are 2-byte aligned only: they are read as 16-bit words.
// Stores are plain vector stores.
#include "../fsq_common.h"
#include "../../../include/fsq_experiment.h"

namespace {

constexpr int SCAN_THREADS = 1024;
constexpr int FRAME_THREADS = 256;
constexpr int REC_H0 = 0, REC_W0 = 8, REC_KEY_H = 120, REC_KEY_W = 124;        // FsqRow of include/fsq.h

__device__ __forceinline__ uint32_t load_u32_a2(const uint8_t* p)
{
    const uint16_t* q = (const uint16_t*)p;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 16);
}
__device__ __forceinline__ double load_f64_a2(const uint8_t* p)
{
    const uint64_t b = (uint64_t)load_u32_a2(p) | ((uint64_t)load_u32_a2(p + 4) << 32);
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    return v;
}

__global__ __launch_bounds__(SCAN_THREADS) void kx_scan(const int32_t* __restrict__ in, int n, int32_t* __restrict__ out,
                                                         int32_t* __restrict__ total)
{
    __shared__ int wsum[SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += SCAN_THREADS) {
        const int i = base + tid;
        const int v = i < n ? max(in[i], 0) : 0;
        const int x = wave_inclusive_scan(v, lane);
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < SCAN_THREADS / 64; k++) {
            const int t = wsum[k];
            if (k < wave) before += t;
            all += t;
        }
        if (i < n) out[i] = carry + before + x - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        out[n] = carry;
        if (total) *total = carry;
    }
}

__global__ __launch_bounds__(FRAME_THREADS) void kx_accept(const uint8_t* __restrict__ records, long long n_records, int record_bytes,
                                                            const int32_t* __restrict__ peaks, const int32_t* __restrict__ rec_start,
                                                            int H, int W, int r, int32_t* __restrict__ keys,
                                                            uint8_t* __restrict__ flags, int32_t* __restrict__ counts,
                                                            int32_t* __restrict__ discarded, int32_t* __restrict__ status)
{
    __shared__ int wkept[FRAME_THREADS / 64];
    const int frame = blockIdx.x, tid = threadIdx.x;
    const int p = peaks[frame];
    const long long a = rec_start[frame];
    int st = FSQ_EXPERIMENT_OK;
    if (p == -1) st = FSQ_EXPERIMENT_REKEY_ASSERT;
    else if (p < -1 || a + p > n_records) st = FSQ_EXPERIMENT_INVALID;
    if (st != FSQ_EXPERIMENT_OK) {                   // (uniform over the block)
        if (tid == 0) { counts[frame] = 0; discarded[frame] = 0; status[frame] = st; }
        return;
    }
    int kept = 0;
    for (int j = tid; j < p; j += FRAME_THREADS) {
        const long long rec = a + j;
        const uint8_t* q = records + rec * record_bytes;
        const int h = (int)load_u32_a2(q + REC_KEY_H), w = (int)load_u32_a2(q + REC_KEY_W);
        // (long long: a key near INT_MAX must not wrap into the image)
        bool ok = 0 <= (long long)h - r && (long long)h + r < H && 0 <= (long long)w - r && (long long)w + r < W;
        if (!ok) {
            const double h0 = load_f64_a2(q + REC_H0), w0 = load_f64_a2(q + REC_W0);
            const bool in_h = (double)r <= h0 && h0 < (double)(H - r);
            const bool in_w = (double)r <= w0 && w0 < (double)(W - r);
            ok = !((!in_h) && in_w);
        }
        keys[2 * rec] = h;
        keys[2 * rec + 1] = w;
        flags[rec] = ok ? 1 : 0;
        kept += ok ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((tid & 63) == 0) wkept[tid >> 6] = kept;
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int k = 0; k < FRAME_THREADS / 64; k++) c += wkept[k];
        counts[frame] = c;
        discarded[frame] = p - c;
        status[frame] = FSQ_EXPERIMENT_OK;
    }
}

__global__ __launch_bounds__(FRAME_THREADS) void kx_compact(const int32_t* __restrict__ peaks, const int32_t* __restrict__ rec_start,
                                                             const int32_t* __restrict__ out_start, const int32_t* __restrict__ status,
                                                             const int32_t* __restrict__ keys, const uint8_t* __restrict__ flags,
                                                             int32_t* __restrict__ hw, int32_t* __restrict__ spot_record)
{
    __shared__ int wcount[FRAME_THREADS / 64];
    const int frame = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (status[frame] != FSQ_EXPERIMENT_OK) return;
    const int p = peaks[frame];
    const long long a = rec_start[frame];
    long long out = out_start[frame];
    for (int base = 0; base < p; base += FRAME_THREADS) {
        const int j = base + tid;
        const long long rec = a + j;
        const bool ok = j < p && flags[rec] != 0;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < FRAME_THREADS / 64; k++) {
            const int t = wcount[k];
            if (k < wave) before += t;
            all += t;
        }
        if (ok) {
            const long long o = out + before + __popcll(m & ((1ull << lane) - 1ull));
            hw[2 * o] = keys[2 * rec];
            hw[2 * o + 1] = keys[2 * rec + 1];
            spot_record[o] = (int32_t)rec;
        }
        out += all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void kx_trace_rows(const int32_t* __restrict__ traces, const int32_t* __restrict__ seq_start,
                                                      const int32_t* __restrict__ field_start, const int32_t* __restrict__ hw,
                                                      int n_seq, int F, long long n_rows, int32_t* __restrict__ trace_hw,
                                                      int32_t* __restrict__ trace_spot, int32_t* __restrict__ trace_seq)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = idx / F;
    const int f = (int)(idx - n * F);
    if (n >= n_rows || n >= seq_start[n_seq]) return;
    int lo = 0, hi = n_seq;                         // the sequence s with seq_start[s] <= n < seq_start[s + 1]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (seq_start[mid] <= n) lo = mid; else hi = mid;
    }
    const int s = lo;
    const long long first = field_start[s], end = field_start[s + 1];
    const long long row = first + (n - seq_start[s]);
    int h = -1, w = -1, at = -1;
    if (row < end) {
        const int spot = traces[row * F + f];
        if (spot >= 0 && first + spot < end) {
            at = (int)(first + spot);
            h = hw[2 * (long long)at];
            w = hw[2 * (long long)at + 1];
        }
    }
    trace_hw[2 * idx] = h;
    trace_hw[2 * idx + 1] = w;
    trace_spot[idx] = at;
    if (f == 0) trace_seq[n] = s;
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

extern "C" int64_t fsq_experiment_spot_table_workspace_bytes(int64_t n_records, int32_t n_frames)
{
    if (n_records < 0 || n_records > 0x7fffffffLL || n_frames < 0) return -1;
    return (int64_t)(2 * align16(((size_t)n_frames + 1) * sizeof(int32_t)) + align16((size_t)n_records * 2 * sizeof(int32_t)) +
                     align16((size_t)n_records));
}

extern "C" int fsq_experiment_spot_table(const uint8_t* d_records, int64_t n_records, int32_t record_bytes, const int32_t* d_peaks,
                                         int32_t n_frames, int32_t H, int32_t W, int32_t spot_size, int32_t* d_hw,
                                         int32_t* d_spot_record, int32_t* d_counts, int32_t* d_discarded, int32_t* d_status,
                                         int32_t* d_n_spots, void* d_ws, int64_t ws_bytes, void* stream)
{
    const int64_t need = fsq_experiment_spot_table_workspace_bytes(n_records, n_frames);
    if (need < 0 || !d_n_spots || H < 1 || W < 1) return FSQ_EINVAL;
    if (record_bytes != 378 && record_bytes != 428) return FSQ_EINVAL;
    if (spot_size < 1 || !(spot_size & 1) || spot_size > 32767) return FSQ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 0) {
        FSQ_HIP_CHECK(hipMemsetAsync(d_n_spots, 0, sizeof(int32_t), s));
        return FSQ_OK;
    }
    if (!d_peaks || !d_counts || !d_discarded || !d_status || !d_ws || ws_bytes < need) return FSQ_EINVAL;
    if (n_records > 0 && (!d_records || !d_hw || !d_spot_record)) return FSQ_EINVAL;
    uint8_t* ws = (uint8_t*)d_ws;
    int32_t* rec_start = (int32_t*)ws;
    ws += align16(((size_t)n_frames + 1) * sizeof(int32_t));
    int32_t* out_start = (int32_t*)ws;
    ws += align16(((size_t)n_frames + 1) * sizeof(int32_t));
    int32_t* keys = (int32_t*)ws;
    ws += align16((size_t)n_records * 2 * sizeof(int32_t));
    uint8_t* flags = ws;
    hipLaunchKernelGGL(kx_scan, dim3(1), dim3(SCAN_THREADS), 0, s, d_peaks, n_frames, rec_start, (int32_t*)nullptr);
    FSQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kx_accept, dim3((unsigned)n_frames), dim3(FRAME_THREADS), 0, s, d_records, (long long)n_records, record_bytes,
                       d_peaks, rec_start, H, W, (spot_size - 1) / 2, keys, flags, d_counts, d_discarded, d_status);
    FSQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kx_scan, dim3(1), dim3(SCAN_THREADS), 0, s, d_counts, n_frames, out_start, d_n_spots);
    FSQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kx_compact, dim3((unsigned)n_frames), dim3(FRAME_THREADS), 0, s, d_peaks, rec_start, out_start, d_status, keys,
                       flags, d_hw, d_spot_record);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_experiment_trace_starts(const int32_t* d_n_traces, int32_t n_seq, int32_t* d_seq_start, void* stream)
{
    if (n_seq < 0 || !d_seq_start || (n_seq > 0 && !d_n_traces)) return FSQ_EINVAL;
    hipLaunchKernelGGL(kx_scan, dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, d_n_traces, n_seq, d_seq_start, (int32_t*)nullptr);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_experiment_trace_rows(const int32_t* d_traces, const int32_t* d_seq_start, const int32_t* d_field_start,
                                         const int32_t* d_hw, int32_t n_seq, int32_t n_frames, int64_t n_rows, int32_t* d_trace_hw,
                                         int32_t* d_trace_spot, int32_t* d_trace_seq, void* stream)
{
    if (n_seq < 1 || n_frames < 1 || n_rows < 0 || n_rows > 0x7fffffffLL) return FSQ_EINVAL;
    const int64_t lanes = n_rows * n_frames;
    if ((lanes + 255) / 256 > 0x7fffffffLL) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_traces || !d_seq_start || !d_field_start || !d_hw || !d_trace_hw || !d_trace_spot || !d_trace_seq) return FSQ_EINVAL;
    hipLaunchKernelGGL(kx_trace_rows, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_traces, d_seq_start,
                       d_field_start, d_hw, n_seq, n_frames, (long long)n_rows, d_trace_hw, d_trace_spot, d_trace_seq);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
