// fsq_sequence.hip - traces of a sequence experiment -> positions, validity, photometries, categories (include/fsq_sequence.h), gfx950.
//
//   kq_accumulate   one lane per (sequence, component): Experiment.accumulate_offsets (flexlibrary.py:567-593), Python's sum left to
//                   right from 0, into the workspace
//   kq_photometry   one wavefront per (trace, frame).  Lane l holds frame l of the trace (<= 64 frames): one ballot gives the
//                   category, every lane restates fill_in_trace / interpolate_spots (flexlibrary.py:1842-2032) for its frame (the
//                   bookends of a hole are the nearest set bits of the category below and above l), two more ballots give the
//                   trace's validity.  Then the wave measures the Spot of ITS frame: the clipped window is spread over the lanes
//                   and held in registers, the crown is summed exactly, the brim's median is found by a binary search on the pixel
//                   VALUE between the brim's own minimum and maximum, counting with one ballot + population count per register (no
//                   cross-lane reduction per step); an even count takes its second middle value from one more count and a minimum.
//                   A (trace, frame) without a Spot reads no pixel.
//   kq_count / kq_compact   traces -> counts per (sequence, pattern): an open-addressing table whose slots hold the index of the
//                   trace that claimed them (the key is read back from the inputs, so a slot is one 32-bit compare-and-swap).
// Every fp64 operation of the geometry is a rounding of its own (-ffp-contract=off).  Stores are plain vector stores.
#include "../fsq_common.h"
#include "../../../include/fsq_sequence.h"

namespace {

constexpr int MAXR = 15;                    // 31 x 31 = 961 pixels <= 16 per lane
constexpr int PER_LANE = 16;
constexpr int COORD_LIMIT = 1 << 29;        // coordinates beyond it count as outside every frame (no int overflow below)

__device__ __forceinline__ long long wave_sum_ll(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned wave_min_u(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ unsigned wave_max_u(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ int ballot_count(bool p) { return __popcll(__ballot(p)); }

struct Window {
    int r0, c0, hc, wc, npx;
};
__device__ __forceinline__ Window clip_window(int H, int W, int h, int w, int radius)
{
    Window q;
    const int r1 = min(H, h + radius + 1), c1 = min(W, w + radius + 1);
    q.r0 = max(0, h - radius);
    q.c0 = max(0, w - radius);
    q.hc = max(r1 - q.r0, 0);
    q.wc = max(c1 - q.c0, 0);
    q.npx = q.hc * q.wc;
    return q;
}

__device__ __forceinline__ double hat_value(long long crown, int ncrown, int nbrim, unsigned m1, unsigned m2)
{
    double med;
    if (nbrim == 0) med = __builtin_nan("");
    else if (nbrim & 1) med = (double)m1;
    else med = ((double)m1 + (double)m2) / 2.0;
    return (double)crown - (double)ncrown * med;
}

// Spot.mexican_hat_photometry_metric with the window in registers (radius <= MAXR); SENT marks a register that holds no brim pixel
template <typename PX>
__device__ double hat_registers(const PX* __restrict__ base, int H, int W, int h, int w, int radius, int brim, int lane)
{
    constexpr unsigned SENT = sizeof(PX) == 2 ? (1u << 16) : (1u << 31);
    const Window q = clip_window(H, W, h, w, radius);
    const int diameter = 2 * radius + 1, nt = (q.npx + 63) >> 6;
    unsigned v[PER_LANE];
    long long crown = 0;
    unsigned vmin = 0xffffffffu, vmax = 0;
#pragma unroll
    for (int t = 0; t < PER_LANE; t++) {
        v[t] = SENT;
        const int i = lane + 64 * t;
        if (t < nt && i < q.npx) {
            const int hh = i / q.wc, ww = i - hh * q.wc;
            const unsigned p = base[(size_t)(q.r0 + hh) * W + (q.c0 + ww)];
            const bool in_crown = (brim <= hh) && (hh < diameter - brim) && (brim <= ww) && (ww < diameter - brim);
            if (in_crown) crown += p;
            else { v[t] = p; vmin = min(vmin, p); vmax = max(vmax, p); }
        }
    }
    crown = wave_sum_ll(crown);
    int nbrim = 0;
#pragma unroll
    for (int t = 0; t < PER_LANE; t++)
        if (t < nt) nbrim += ballot_count(v[t] != SENT);
    const int ncrown = q.npx - nbrim;
    if (nbrim == 0) return hat_value(crown, ncrown, 0, 0, 0);
    unsigned lo = wave_min_u(vmin), hi = wave_max_u(vmax);
    auto count_le = [&](unsigned x) {
        int c = 0;
#pragma unroll
        for (int t = 0; t < PER_LANE; t++)
            if (t < nt) c += ballot_count(v[t] <= x);
        return c;
    };
    const int rank = (nbrim - 1) / 2;                  // lower middle value (the middle one of an odd count), 0-based
    while (lo < hi) {                                   // smallest x with #{brim <= x} >= rank + 1
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (count_le(mid) >= rank + 1) hi = mid; else lo = mid + 1;
    }
    unsigned m2 = lo;
    if (!(nbrim & 1) && count_le(lo) < rank + 2) {     // the upper middle value is the next larger brim pixel
        unsigned nx = 0xffffffffu;
#pragma unroll
        for (int t = 0; t < PER_LANE; t++)
            if (t < nt && v[t] > lo && v[t] != SENT) nx = min(nx, v[t]);
        m2 = wave_min_u(nx);
    }
    return hat_value(crown, ncrown, nbrim, lo, m2);
}

// the same for any radius: the window is read again (from L1 / L2) for every step of the search
template <typename PX>
__device__ double hat_any(const PX* __restrict__ base, int H, int W, int h, int w, int radius, int brim, int lane)
{
    const Window q = clip_window(H, W, h, w, radius);
    const int diameter = 2 * radius + 1;
    auto in_crown = [&](int hh, int ww) { return (brim <= hh) && (hh < diameter - brim) && (brim <= ww) && (ww < diameter - brim); };
    long long crown = 0, nb = 0;
    unsigned vmin = 0xffffffffu, vmax = 0;
    for (int i = lane; i < q.npx; i += 64) {
        const int hh = i / q.wc, ww = i - hh * q.wc;
        const unsigned p = base[(size_t)(q.r0 + hh) * W + (q.c0 + ww)];
        if (in_crown(hh, ww)) crown += p;
        else { nb++; vmin = min(vmin, p); vmax = max(vmax, p); }
    }
    crown = wave_sum_ll(crown);
    const int nbrim = (int)wave_sum_ll(nb), ncrown = q.npx - nbrim;
    if (nbrim == 0) return hat_value(crown, ncrown, 0, 0, 0);
    unsigned lo = wave_min_u(vmin), hi = wave_max_u(vmax);
    auto count_le = [&](unsigned x) {
        long long c = 0;
        for (int i = lane; i < q.npx; i += 64) {
            const int hh = i / q.wc, ww = i - hh * q.wc;
            if (!in_crown(hh, ww)) c += ((unsigned)base[(size_t)(q.r0 + hh) * W + (q.c0 + ww)] <= x);
        }
        return (int)wave_sum_ll(c);
    };
    const int rank = (nbrim - 1) / 2;
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (count_le(mid) >= rank + 1) hi = mid; else lo = mid + 1;
    }
    unsigned m2 = lo;
    if (!(nbrim & 1) && count_le(lo) < rank + 2) {
        unsigned nx = 0xffffffffu;
        for (int i = lane; i < q.npx; i += 64) {
            const int hh = i / q.wc, ww = i - hh * q.wc;
            const unsigned p = base[(size_t)(q.r0 + hh) * W + (q.c0 + ww)];
            if (!in_crown(hh, ww) && p > lo) nx = min(nx, p);
        }
        m2 = wave_min_u(nx);
    }
    return hat_value(crown, ncrown, nbrim, lo, m2);
}

// Spot.simple_photometry_metric: the sum of the clipped window (exact: < 2^53)
template <typename PX>
__device__ double window_sum(const PX* __restrict__ base, int H, int W, int h, int w, int radius, int lane)
{
    const Window q = clip_window(H, W, h, w, radius);
    long long s = 0;
    for (int i = lane; i < q.npx; i += 64) {
        const int hh = i / q.wc, ww = i - hh * q.wc;
        s += (unsigned)base[(size_t)(q.r0 + hh) * W + (q.c0 + ww)];
    }
    return (double)wave_sum_ll(s);
}

__global__ void __launch_bounds__(256) kq_accumulate(const double* __restrict__ off, int n_seq, int F, double* __restrict__ cum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;       // (sequence, component)
    if (i >= 2 * n_seq) return;
    const int s = i >> 1, c = i & 1;
    double acc = 0.0;
    for (int f = 0; f < F; f++) {
        acc = acc + off[((size_t)s * F + f) * 2 + c];
        cum[((size_t)s * F + f) * 2 + c] = acc;
    }
}

// int(py2_round(p)); false when p is not a coordinate any frame could hold
__device__ __forceinline__ bool round_coordinate(double p, int* out)
{
    const double r = round(p);                          // half away from zero, as Python 2's round
    if (!(r > -(double)COORD_LIMIT && r < (double)COORD_LIMIT)) return false;
    *out = (int)r;
    return true;
}

template <typename PX>
__global__ void __launch_bounds__(256) kq_photometry(const PX* __restrict__ frames, int n_seq, int F, int H, int W,
                                                      const int32_t* __restrict__ trace_hw, const int32_t* __restrict__ trace_seq,
                                                      long long n_traces, const double* __restrict__ cum, int radius, int brim,
                                                      int spot_r, int method, int interpolate, int32_t* __restrict__ out_hw,
                                                      double* __restrict__ out_phot, uint8_t* __restrict__ out_flags,
                                                      unsigned long long* __restrict__ out_category, uint8_t* __restrict__ out_valid)
{
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_traces * F) return;
    const long long trace = g / F;
    const int f = (int)(g - trace * F);
    const int seq = trace_seq[trace];
    const bool seq_ok = seq >= 0 && seq < n_seq;
    const int wr = method == FSQ_SEQUENCE_SIMPLE ? spot_r : radius;      // radius of the photometry window

    // ---- lane l = frame l of the trace ----
    int th = -1, tw = -1;
    if (lane < F && seq_ok) {
        th = trace_hw[(trace * F + lane) * 2];
        tw = trace_hw[(trace * F + lane) * 2 + 1];
    }
    const bool det = th >= 0 && tw >= 0;
    const unsigned long long mask = __ballot(det);
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const unsigned long long above = lane == 63 ? 0ull : mask & (~0ull << (lane + 1));
    const bool has_a = below != 0, has_b = above != 0;
    const int a = has_a ? 63 - __clzll((long long)below) : 0;
    const int b = has_b ? __ffsll((long long)above) - 1 : F - 1;
    const int ah = __shfl(th, a), aw = __shfl(tw, a), bh = __shfl(th, b), bw = __shfl(tw, b);
    int ph = th, pw = tw;
    bool exist = det, interpolated = false;
    if (!det && lane < F && interpolate && mask != 0ull) {
        const double* c = cum + (size_t)seq * F * 2;
        const double ca_h = c[2 * a], ca_w = c[2 * a + 1], cb_h = c[2 * b], cb_w = c[2 * b + 1];
        const double ci_h = c[2 * lane], ci_w = c[2 * lane + 1];
        double start_h, start_w, stop_h, stop_w;
        if (has_b) {                                    // stop = hw[b] + co(a, b); a leading hole starts there too (a = 0)
            stop_h = (double)bh + (ca_h - cb_h);
            stop_w = (double)bw + (ca_w - cb_w);
        }
        if (has_a) { start_h = (double)ah; start_w = (double)aw; }
        else { start_h = stop_h; start_w = stop_w; }
        if (!has_b) { stop_h = start_h; stop_w = start_w; }            // trailing hole
        const double n = (double)(b - a), k = (double)(lane - a);
        const double inc_h = (stop_h - start_h) / n, inc_w = (stop_w - start_w) / n;
        double p_h = start_h + inc_h * k, p_w = start_w + inc_w * k;
        p_h = p_h + (ci_h - ca_h);
        p_w = p_w + (ci_w - ca_w);
        int ih, iw;
        if (round_coordinate(p_h, &ih) && round_coordinate(p_w, &iw) && spot_r <= ih && ih < H - spot_r && spot_r <= iw &&
            iw < W - spot_r) {
            ph = ih; pw = iw; exist = true; interpolated = true;
        }
    }
    if (exist && (ph >= COORD_LIMIT || pw >= COORD_LIMIT)) { ph = pw = COORD_LIMIT; }    // (a detected Spot far outside: empty window)
    const bool inside = exist && ph - wr >= 0 && ph + wr < H && pw - wr >= 0 && pw + wr < W;
    const unsigned long long full = F == 64 ? ~0ull : (1ull << F) - 1ull;
    const bool valid = seq_ok && __ballot(inside) == full;
    const int flags = (det ? FSQ_SEQUENCE_DETECTED : 0) | (interpolated ? FSQ_SEQUENCE_INTERPOLATED : 0) |
                      (inside ? FSQ_SEQUENCE_WINDOW_INSIDE : 0);

    // ---- the wave's own frame ----
    const int mh = __shfl(ph, f), mw = __shfl(pw, f), mflags = __shfl(flags, f);
    const bool mexist = (mflags & (FSQ_SEQUENCE_DETECTED | FSQ_SEQUENCE_INTERPOLATED)) != 0;
    if (lane == 0) {
        out_hw[g * 2] = mexist ? mh : -1;
        out_hw[g * 2 + 1] = mexist ? mw : -1;
        out_flags[g] = (uint8_t)mflags;
        if (f == 0) {
            out_category[trace] = mask;
            out_valid[trace] = valid ? 1 : 0;
        }
        if (!mexist) out_phot[g] = __builtin_nan("");
    }
    if (!mexist) return;
    const PX* base = frames + ((size_t)seq * F + f) * H * W;
    double v;
    if (method == FSQ_SEQUENCE_SIMPLE) v = window_sum(base, H, W, mh, mw, wr, lane);
    else if (radius <= MAXR) v = hat_registers(base, H, W, mh, mw, radius, brim, lane);
    else v = hat_any(base, H, W, mh, mw, radius, brim, lane);
    if (lane == 0) out_phot[g] = v;
}

__device__ __forceinline__ unsigned hash_key(unsigned long long pattern, int seq)
{
    unsigned long long x = pattern ^ ((unsigned long long)(unsigned)seq * 0x9E3779B97F4A7C15ull);
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (unsigned)x;
}

__global__ void __launch_bounds__(256) kq_count(const unsigned long long* __restrict__ category, const int32_t* __restrict__ trace_seq,
                                                 const uint8_t* __restrict__ select, long long n, int* owner, int* count, int* first,
                                                 unsigned cap_mask)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (select && !select[i]) return;
    const unsigned long long key = category[i];
    const int s = trace_seq[i];
    unsigned slot = hash_key(key, s) & cap_mask;
    for (;;) {                                          // the table has more than twice as many slots as traces: ends
        int o = atomicCAS(&owner[slot], -1, (int)i);
        if (o == -1) o = (int)i;
        if (category[o] == key && trace_seq[o] == s) {
            atomicAdd(&count[slot], 1);
            atomicMin(&first[slot], (int)i);
            return;
        }
        slot = (slot + 1) & cap_mask;
    }
}

__global__ void __launch_bounds__(256) kq_compact(const unsigned long long* __restrict__ category, const int32_t* __restrict__ trace_seq,
                                                   const int* __restrict__ owner, const int* __restrict__ count,
                                                   const int* __restrict__ first, unsigned cap, int32_t* __restrict__ g_seq,
                                                   unsigned long long* __restrict__ g_pattern, int32_t* __restrict__ g_count,
                                                   int32_t* __restrict__ g_first, int* n_groups)
{
    const unsigned slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= cap) return;
    const int o = owner[slot];
    if (o < 0) return;
    const int j = atomicAdd(n_groups, 1);
    g_seq[j] = trace_seq[o];
    g_pattern[j] = category[o];
    g_count[j] = count[slot];
    g_first[j] = first[slot];
}

unsigned table_capacity(int64_t n)
{
    unsigned cap = 64;
    while ((int64_t)cap < 2 * n + 1) cap <<= 1;
    return cap;
}

template <typename PX>
int sequence_launch(const PX* d_frames, int32_t n_seq, int32_t F, int32_t H, int32_t W, const int32_t* d_trace_hw,
                    const int32_t* d_trace_seq, int64_t n_traces, const double* d_offsets, int32_t radius, int32_t brim_size,
                    int32_t spot_size, int32_t method, int32_t interpolate, int32_t* d_hw, double* d_phot, uint8_t* d_flags,
                    uint64_t* d_category, uint8_t* d_trace_valid, void* d_ws, int64_t ws_bytes, void* stream)
{
    if (n_traces < 0 || n_seq < 1 || F < 1 || H < 1 || W < 1 || brim_size < 0 || radius < 0 || radius > 16383) return FSQ_EINVAL;
    if (spot_size < 1 || !(spot_size & 1) || spot_size > 32767) return FSQ_EINVAL;
    if (method != FSQ_SEQUENCE_MEXICAN_HAT && method != FSQ_SEQUENCE_SIMPLE) return FSQ_EINVAL;
    if (F > FSQ_SEQUENCE_MAX_FRAMES) return FSQ_ENOTIMPL;
    if (H >= COORD_LIMIT || W >= COORD_LIMIT) return FSQ_EINVAL;
    const int64_t waves = n_traces * F;
    if ((waves + 3) / 4 > 0x7fffffffLL) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_frames || !d_trace_hw || !d_trace_seq || !d_offsets || !d_hw || !d_phot || !d_flags || !d_category || !d_trace_valid || !d_ws)
        return FSQ_EINVAL;
    if (ws_bytes < fsq_sequence_workspace_bytes(n_seq, F)) return FSQ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* cum = (double*)d_ws;
    hipLaunchKernelGGL(kq_accumulate, dim3((unsigned)((2 * (int64_t)n_seq + 255) / 256)), dim3(256), 0, s, d_offsets, n_seq, F, cum);
    FSQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kq_photometry<PX>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, d_frames, n_seq, F, H, W, d_trace_hw,
                       d_trace_seq, (long long)n_traces, cum, radius, brim_size, (spot_size - 1) / 2, method, interpolate ? 1 : 0, d_hw,
                       d_phot, d_flags, (unsigned long long*)d_category, d_trace_valid);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

}  // namespace

extern "C" int64_t fsq_sequence_workspace_bytes(int32_t n_seq, int32_t n_frames)
{
    if (n_seq < 1 || n_frames < 1) return -1;
    return (int64_t)n_seq * n_frames * 2 * (int64_t)sizeof(double);
}

extern "C" int fsq_sequence_photometry(const uint16_t* d_frames, int32_t n_seq, int32_t n_frames, int32_t H, int32_t W,
                                       const int32_t* d_trace_hw, const int32_t* d_trace_seq, int64_t n_traces,
                                       const double* d_offsets, int32_t radius, int32_t brim_size, int32_t spot_size, int32_t method,
                                       int32_t interpolate, int32_t* d_hw, double* d_phot, uint8_t* d_flags, uint64_t* d_category,
                                       uint8_t* d_trace_valid, void* d_ws, int64_t ws_bytes, void* stream)
{
    return sequence_launch(d_frames, n_seq, n_frames, H, W, d_trace_hw, d_trace_seq, n_traces, d_offsets, radius, brim_size, spot_size,
                           method, interpolate, d_hw, d_phot, d_flags, d_category, d_trace_valid, d_ws, ws_bytes, stream);
}

extern "C" int fsq_sequence_photometry_u32(const uint32_t* d_frames, int32_t n_seq, int32_t n_frames, int32_t H, int32_t W,
                                           const int32_t* d_trace_hw, const int32_t* d_trace_seq, int64_t n_traces,
                                           const double* d_offsets, int32_t radius, int32_t brim_size, int32_t spot_size,
                                           int32_t method, int32_t interpolate, int32_t* d_hw, double* d_phot, uint8_t* d_flags,
                                           uint64_t* d_category, uint8_t* d_trace_valid, void* d_ws, int64_t ws_bytes, void* stream)
{
    return sequence_launch(d_frames, n_seq, n_frames, H, W, d_trace_hw, d_trace_seq, n_traces, d_offsets, radius, brim_size, spot_size,
                           method, interpolate, d_hw, d_phot, d_flags, d_category, d_trace_valid, d_ws, ws_bytes, stream);
}

extern "C" int64_t fsq_sequence_category_counts_workspace_bytes(int64_t n_traces)
{
    if (n_traces < 0 || n_traces > (1LL << 29)) return -1;
    return 3 * (int64_t)table_capacity(n_traces) * (int64_t)sizeof(int);
}

extern "C" int fsq_sequence_category_counts(const uint64_t* d_category, const int32_t* d_trace_seq, const uint8_t* d_select,
                                            int64_t n_traces, int32_t* d_group_seq, uint64_t* d_group_pattern,
                                            int32_t* d_group_count, int32_t* d_group_first, int32_t* d_n_groups, void* d_ws,
                                            int64_t ws_bytes, void* stream)
{
    const int64_t need = fsq_sequence_category_counts_workspace_bytes(n_traces);
    if (need < 0 || !d_n_groups) return FSQ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    FSQ_HIP_CHECK(hipMemsetAsync(d_n_groups, 0, sizeof(int32_t), s));
    if (n_traces == 0) return FSQ_OK;
    if (!d_category || !d_trace_seq || !d_group_seq || !d_group_pattern || !d_group_count || !d_group_first || !d_ws || ws_bytes < need)
        return FSQ_EINVAL;
    const unsigned cap = table_capacity(n_traces);
    int* owner = (int*)d_ws;
    int* count = owner + cap;
    int* first = count + cap;
    FSQ_HIP_CHECK(hipMemsetAsync(owner, 0xff, (size_t)cap * sizeof(int), s));           // -1: free
    FSQ_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)cap * sizeof(int), s));
    FSQ_HIP_CHECK(hipMemsetAsync(first, 0x7f, (size_t)cap * sizeof(int), s));           // above every trace index (<= 2^29)
    hipLaunchKernelGGL(kq_count, dim3((unsigned)((n_traces + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)d_category,
                       d_trace_seq, d_select, (long long)n_traces, owner, count, first, cap - 1u);
    FSQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kq_compact, dim3((cap + 255u) / 256u), dim3(256), 0, s, (const unsigned long long*)d_category, d_trace_seq, owner,
                       count, first, cap, d_group_seq, (unsigned long long*)d_group_pattern, d_group_count, d_group_first, d_n_groups);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
