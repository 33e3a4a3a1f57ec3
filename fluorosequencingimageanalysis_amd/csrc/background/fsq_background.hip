// fsq_background.hip - the iterative background correction of signal counts (include/fsq_background.h):
// MCsimlib.iterative_peak_finding_v3 (:5932-6019) for P independent problems, with the reference's bits.
//
// kbg_neighbours, one lane per key, once per call: the key's neighbours in itertools.product order, those out of range or
//   excluded as multidrop left out, each the index of its key (a binary search of the problem's sorted codes) or -1 (absent).
// kbg_first, one 256-thread workgroup per problem, once per call: the z-scores of the caller's percents, the first-in-order
//   arg-max of z and the threshold test, the trial list by an ordered compaction (list_trials; every later pass gets them
//   from the tail of the pass before it: z-scores are those of the percents the last pass left, :5948 comes before :5962).
// kbg_head, one 256-thread workgroup per problem: the undefined keys interpolated one after the other (the workgroup gathers
//   the neighbours' counts into LDS, lane 0 adds them as numpy's pairwise sum does); the base sum, tile by tile through LDS,
//   lane 0 adding in order and noting the sum before every key; percents; then the stop the z-scores asked for.
// kbg_trials, one wavefront per 64 trials: lane t interpolates its key's count (numpy's pairwise sum over its neighbours), then
//   starts from the noted sum before the first substituted key of its wave and adds the filtered counts in order with its own
//   count replaced.  The walk index is the wave's, so the counts come through
//   uniform loads, once per wave.
// kbg_tail, one workgroup per problem: first-in-order arg-max of the differences, the <= 0 test, the acceptance, the < 0.001
//   test against the state after the previous acceptance, the percents from the winner's own total, and list_trials for
//   the next pass.
// A problem that stops writes its rounded counts, reason and counters and sets its done flag (a stop the head finds is
// noted in the problem's state and carried out by the tail of the same pass); every kernel returns at once on that flag.  No workgroup waits for another, nothing spins on memory.
//
// Bounds: every index read from a caller's list is used only where 0 <= index < the problem's keys; a neighbour entry is
// written only inside the key's room nb_off[k] .. nb_off[k + 1]; offsets are used only where they ascend inside their arrays.
#include <hip/hip_runtime.h>
#include <math.h>

#include <vector>

#include "../fsq_common.h"
#include "../../../include/fsq_background.h"
#include "../stepfit/fsq_pairwise.h"
#include "../stepfit/fsq_plateau_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int TRIAL_THREADS = FSQ_BACKGROUND_TRIAL_THREADS;
constexpr int TILE = FSQ_BACKGROUND_TILE;
constexpr int MAX_DROPS = FSQ_BACKGROUND_MAX_DROPS;
constexpr int MAX_NEIGHBOURS = 728;                                // 3^MAX_DROPS - 1
static_assert(TRIAL_THREADS == WAVE, "one wavefront per trial workgroup: its walk index is uniform");
static_assert(MAX_NEIGHBOURS <= TILE && TILE % THREADS == 0, "one LDS array serves the gather and the tile");

typedef unsigned long long u64;

struct State {                                                     // per problem, zeroed before the first pass
    int passes, accepted, n_trials, has_prior, und_written, zero_trial;
    int reason, next;                                              // a stop the head found, which the tail carries out; the stop the z-scores ask for
    double total;
};

struct Work {                                                      // the workspace
    State* state;
    int* done;
    int* nb_cnt;
    int* nb;
    double* prefix;
    double* prior;
    double* z;
    double* interp;
    double* diff;
    double* ttotal;
    int* trial;
};

// the problem's view of the arguments: lengths are 0 where an offset pair does not ascend inside its array
struct Prob {
    long long k0, d0;
    int N, D, U;
    const int* und;
};

__device__ __forceinline__ void span(const int64_t* off, int p, long long limit, long long* o, int* n)
{
    const long long a = off[p], b = off[p + 1];
    const bool ok = a >= 0 && b >= a && b <= limit && b - a < (1ll << 31);
    *o = ok ? a : 0;
    *n = ok ? (int)(b - a) : 0;
}

__device__ __forceinline__ Prob problem_of(const FsqBackgroundArgs& A, int p, bool first)
{
    Prob q;
    span(A.key_off, p, A.n_keys, &q.k0, &q.N);
    span(A.def_off, p, A.n_defined, &q.d0, &q.D);
    long long u0;
    span(first ? A.first_off : A.rest_off, p, first ? A.n_first : A.n_rest, &u0, &q.U);
    q.und = (first ? A.und_first : A.und_rest) + u0;
    return q;
}

// (:5787-5790) pow is glibc's, the division and the square root are IEEE
__device__ __forceinline__ double z_score(double bp, double ap, double sp)
{
    const double d = bp - ap;
    const double m = cs_pow2(d) / cs_pow2(sp);
    return copysign(__dsqrt_rn(m), d);
}

// pflib._py2_round as an int64; INT64_MIN where the count is not finite or beyond int64
__device__ __forceinline__ long long rounded_of(double x)
{
    const double r = x >= 0.0 ? floor(x + 0.5) : ceil(x - 0.5);
    if (!(r > -9.2e18 && r < 9.2e18)) return (long long)0x8000000000000000ull;
    return (long long)r;
}

// Python's max(d, key=d.get) over a[0 .. n): the first largest value; a NaN at 0 stays, a NaN elsewhere never wins.
// n >= 1; the whole workgroup calls it; sv / si hold THREADS entries.
__device__ int first_argmax(const double* a, int n, double* sv, int* si)
{
    const int tid = threadIdx.x;
    double bv = 0.0;
    int bi = -1;
    for (int i = tid; i < n; i += THREADS) {
        const double v = a[i];
        if (v == v && (bi < 0 || v > bv)) { bv = v; bi = i; }
    }
    sv[tid] = bv;
    si[tid] = bi;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double v2 = sv[tid + s];
            const int i2 = si[tid + s], i1 = si[tid];
            if (i2 >= 0 && (i1 < 0 || v2 > sv[tid] || (v2 == sv[tid] && i2 < i1))) { sv[tid] = v2; si[tid] = i2; }
        }
        __syncthreads();
    }
    const double first = a[0];
    const int r = (first != first || si[0] < 0) ? 0 : si[0];
    __syncthreads();                                               // (sv / si are free again)
    return r;
}

// the problem stops: rounded counts, reason, counters, the done flag.  Uniform over the workgroup.
__device__ void finish(const FsqBackgroundArgs& A, const Work& W, const Prob& q, int p, int reason)
{
    __syncthreads();
    for (int j = threadIdx.x; j < q.N; j += THREADS) A.rounded[q.k0 + j] = rounded_of(A.count[q.k0 + j]);
    if (threadIdx.x == 0) {
        A.stop_reason[p] = reason;
        A.n_passes[p] = W.state[p].passes;
        A.n_accepted[p] = W.state[p].accepted;
        W.done[p] = 1;
    }
}

// The z-scores of the percents as they stand (:5948-5952, :5787-5790), the stop they ask for (:5968-5972: none defined, or the
// first-in-order largest <= the threshold) and the trials in order (:5982-5984, an ordered compaction): what the next pass
// needs before anything else, made by the tail of the pass before it, and once before the first pass.  The whole workgroup
// calls it; percent must be visible to it.
__device__ void list_trials(const FsqBackgroundArgs& A, const Work& W, const Prob& q, int p, double* s_rv, int* s_ri, int* s_wcnt)
{
    const int tid = threadIdx.x;
    State& st = W.state[p];
    const double* percent = A.percent + q.k0;
    const int* def_key = A.def_key + q.d0;
    double* z = W.z + q.d0;
    const double thr = A.sigma_threshold[p];
    if (q.D == 0) {
        if (tid == 0) { st.next = FSQ_BACKGROUND_NO_DEFINED; st.n_trials = 0; }
        return;
    }
    for (int i = tid; i < q.D; i += THREADS) {
        const int k = def_key[i];
        z[i] = z_score(k >= 0 && k < q.N ? percent[k] : 0.0, A.def_avg[q.d0 + i], A.def_std[q.d0 + i]);
    }
    __syncthreads();                                               // (z is the workgroup's)
    const int best = first_argmax(z, q.D, s_rv, s_ri);
    if (z[best] <= thr) {
        if (tid == 0) { st.next = FSQ_BACKGROUND_THRESHOLD; st.n_trials = 0; }
        return;
    }
    int* trial = W.trial + q.d0;
    int run = 0;
    for (int base = 0; base < q.D; base += THREADS) {
        const int i = base + tid;
        bool flag = false;
        if (i < q.D) {
            const int k = def_key[i];
            flag = k >= 0 && k < q.N && !(z[i] <= thr);
        }
        const u64 ballot = __ballot(flag);
        const int wave = tid / WAVE, lane = tid % WAVE;
        if (lane == 0) s_wcnt[wave] = __popcll(ballot);
        __syncthreads();
        int off = run, all = 0;
        for (int w = 0; w < THREADS / WAVE; w++) {
            if (w < wave) off += s_wcnt[w];
            all += s_wcnt[w];
        }
        if (flag) trial[off + __popcll(ballot & ((1ull << lane) - 1ull))] = i;
        run += all;
        __syncthreads();
    }
    if (tid == 0) { st.next = 0; st.n_trials = run; }
}

__global__ void __launch_bounds__(THREADS) kbg_first(FsqBackgroundArgs A, Work W)
{
    __shared__ double s_rv[THREADS];
    __shared__ int s_ri[THREADS];
    __shared__ int s_wcnt[THREADS / WAVE];
    list_trials(A, W, problem_of(A, blockIdx.x, false), blockIdx.x, s_rv, s_ri, s_wcnt);
}

__global__ void __launch_bounds__(THREADS) kbg_neighbours(FsqBackgroundArgs A, Work W)
{
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= A.n_keys) return;
    int a = 0, b = A.n_problems + 1;                               // #{j <= P : key_off[j] <= g}
    while (a < b) {
        const int mid = a + ((b - a) >> 1);
        if (A.key_off[mid] <= g) a = mid + 1; else b = mid;
    }
    const int p = a - 1;
    W.nb_cnt[g] = 0;
    if (p < 0 || p >= A.n_problems) return;
    const Prob q = problem_of(A, p, true);
    if (g < q.k0 || g >= q.k0 + q.N) return;
    const u64 code = A.code[g];
    const int d = (int)((code >> 48) & 7);
    const long long room0 = A.nb_off[g], room1 = A.nb_off[g + 1];
    if (d < 1 || d > MAX_DROPS || room0 < 0 || room1 < room0 || room1 > A.n_neighbours) return;
    const int cycles = A.num_cycles[p];
    const bool multidrop = A.include_multidrop[p] != 0;
    int nq = 1;
    for (int i = 0; i < d; i++) nq *= 3;
    const u64* sorted = (const u64*)A.sorted_code + q.k0;
    int cnt = 0;
    for (int e = 0; e < nq; e++) {
        if (e == (nq - 1) / 2) continue;                           // the key itself
        u64 c = code & ~0xffffffffffffull;
        bool ok = true;
        int rest = e, pw = nq;
        int pos[MAX_DROPS];
#pragma unroll
        for (int i = 0; i < MAX_DROPS; i++) {
            pos[i] = -1 - i;                                       // (distinct placeholders beyond d)
            if (i < d) {
                pw /= 3;
                const int digit = rest / pw;                       // the first position varies slowest
                rest -= digit * pw;
                const int v = (int)((code >> (8 * i)) & 255) + digit - 1;
                ok = ok && v > 0 && v <= cycles;
                pos[i] = v;
                c |= (u64)(v & 255) << (8 * i);
            }
        }
        if (!multidrop) {
#pragma unroll
            for (int i = 0; i < MAX_DROPS; i++)
#pragma unroll
                for (int j = i + 1; j < MAX_DROPS; j++) ok = ok && pos[i] != pos[j];
        }
        if (!ok) continue;
        int lo = 0, hi = q.N;                                      // the first sorted code >= c
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (sorted[mid] < c) lo = mid + 1; else hi = mid;
        }
        int idx = -1;
        if (lo < q.N && sorted[lo] == c) {
            idx = A.sorted_index[q.k0 + lo];
            if (idx < 0 || idx >= q.N) idx = -1;
        }
        if (room0 + cnt < room1) W.nb[room0 + cnt++] = idx;
    }
    W.nb_cnt[g] = cnt;
}

__global__ void __launch_bounds__(THREADS) kbg_head(FsqBackgroundArgs A, Work W)
{
    __shared__ double s_val[TILE];
    __shared__ unsigned char s_flt[TILE];
    __shared__ int s_wcnt[1];
    __shared__ double s_total;
    const int tid = threadIdx.x, p = blockIdx.x;
    if (W.done[p]) return;
    State& st = W.state[p];
    const int pass = st.passes;
    const Prob q = problem_of(A, p, pass == 0);
    if (pass >= A.max_iterations) {
        if (tid == 0) st.reason = FSQ_BACKGROUND_MAX_ITERATIONS;
        return;
    }
    double* count = A.count + q.k0;
    double* percent = A.percent + q.k0;
    const unsigned char* filter = A.filter + q.k0;
    // ---- the undefined keys, one after the other (:5953-5961)
    const int written = st.und_written;
    for (int u = 0; u < q.U; u++) {
        const int k = q.und[u];
        if (k < 0 || k >= q.N) continue;                           // (uniform)
        if (tid == 0 && A.undefined_bp) {
            const long long slot = (long long)written + u;
            if (slot < A.undefined_cap) A.undefined_bp[(long long)p * A.undefined_cap + slot] = percent[k];
            else A.overflow[p] |= FSQ_BACKGROUND_OVERFLOW_UNDEFINED;
        }
        const int* nb = W.nb + A.nb_off[q.k0 + k];
        const int m = min(W.nb_cnt[q.k0 + k], MAX_NEIGHBOURS);
        for (int e = tid; e < m; e += THREADS) {
            const int idx = nb[e];
            s_val[e] = idx >= 0 ? count[idx] : 0.0;
        }
        __syncthreads();
        if (tid == 0) count[k] = np_mean_flat<3>(s_val, m);
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) st.und_written = written + q.U;
    if (tid == 0) st.passes = pass + 1;
    // ---- the base sum in order, and the sum before every key (:5655)
    double total = 0.0;
    int n_filtered = 0;
    for (int t0 = 0; t0 < q.N; t0 += TILE) {
        const int n = min(TILE, q.N - t0);
        for (int e = tid; e < n; e += THREADS) {
            s_val[e] = count[t0 + e];
            s_flt[e] = filter[t0 + e];
        }
        __syncthreads();
        if (tid == 0) {
            double* prefix = W.prefix + q.k0 + t0;
            for (int e = 0; e < n; e++) {
                prefix[e] = total;
                if (s_flt[e]) { total += s_val[e]; n_filtered++; }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        s_total = total;
        s_wcnt[0] = n_filtered;
        st.total = total;
    }
    __syncthreads();
    total = s_total;
    n_filtered = s_wcnt[0];
    __syncthreads();
    if (n_filtered > 0 && total == 0.0) {                          // float(count) / 0
        if (tid == 0) st.reason = FSQ_BACKGROUND_ZERO_TOTAL;
        return;
    }
    for (int j = tid; j < q.N; j += THREADS) percent[j] = filter[j] ? count[j] / total : 0.0;
    // ---- the stops before the trials (:5968-5972), as the z-scores of the percents the last pass left ask for
    if (tid == 0 && st.next) st.reason = st.next;
}

__global__ void __launch_bounds__(TRIAL_THREADS) kbg_trials(FsqBackgroundArgs A, Work W)
{
    const int p = blockIdx.y, lane = threadIdx.x;
    if (W.done[p] || W.state[p].reason) return;
    const State& st = W.state[p];
    const int T = st.n_trials;
    const int t = blockIdx.x * TRIAL_THREADS + lane;
    if (blockIdx.x * TRIAL_THREADS >= T) return;                   // (uniform)
    const Prob q = problem_of(A, p, false);
    const double* count = A.count + q.k0;
    const unsigned char* filter = A.filter + q.k0;
    const bool active = t < T && T <= q.D;
    int i = 0, k = 0;
    double v = 0.0;
    bool filtered = false;
    if (active) {
        i = W.trial[q.d0 + t];
        k = A.def_key[q.d0 + i];
        filtered = filter[k] != 0;
        // the interpolated count (:5973-5980): np.mean of the neighbours' counts, absent ones 0
        const int* nb = W.nb + A.nb_off[q.k0 + k];
        const int m = min(W.nb_cnt[q.k0 + k], MAX_NEIGHBOURS);
        v = (0.0 + pw_sum_flat<3>([nb, count](int e) { const int idx = nb[e]; return idx >= 0 ? count[idx] : 0.0; }, 0, m)) / (double)m;
        W.interp[q.d0 + t] = v;
    }
    const int pos = filtered ? k : q.N;                            // the key whose count this lane replaces
    int jmin = pos;
#pragma unroll
    for (int s = WAVE / 2; s > 0; s >>= 1) jmin = min(jmin, __shfl_xor(jmin, s, WAVE));
    jmin = __builtin_amdgcn_readfirstlane(jmin);
    double acc = jmin < q.N ? W.prefix[q.k0 + jmin] : 0.0;
    for (int j = jmin; j < q.N; j++) {                             // j is the wave's: uniform loads
        if (!filter[j]) continue;
        const double c = count[j];
        acc += j == pos ? v : c;
    }
    if (!active) return;
    const double total = filtered ? acc : st.total;
    if (filtered && total == 0.0) W.state[p].zero_trial = 1;       // (the reference's float(count) / 0; every lane writes the same 1)
    const double bp = filtered ? v / total : 0.0;                  // (a key outside the filter has no percent)
    W.diff[q.d0 + t] = W.z[q.d0 + i] - z_score(bp, A.def_avg[q.d0 + i], A.def_std[q.d0 + i]);
    W.ttotal[q.d0 + t] = total;
}

__global__ void __launch_bounds__(THREADS) kbg_tail(FsqBackgroundArgs A, Work W)
{
    __shared__ double s_rv[THREADS];
    __shared__ int s_ri[THREADS];
    __shared__ int s_wcnt[THREADS / WAVE];
    const int tid = threadIdx.x, p = blockIdx.x;
    if (W.done[p]) return;
    State& st = W.state[p];
    const Prob q = problem_of(A, p, false);
    if (st.reason) {                                               // (the head's stop)
        finish(A, W, q, p, st.reason);
        return;
    }
    const int T = min(st.n_trials, q.D);
    if (T < 1) {                                                   // (the largest z is itself a trial)
        finish(A, W, q, p, FSQ_BACKGROUND_NO_IMPROVEMENT);
        return;
    }
    if (st.zero_trial) {
        finish(A, W, q, p, FSQ_BACKGROUND_ZERO_TOTAL);
        return;
    }
    const double* diff = W.diff + q.d0;
    const int b = first_argmax(diff, T, s_rv, s_ri);
    if (diff[b] <= 0.0) {
        finish(A, W, q, p, FSQ_BACKGROUND_NO_IMPROVEMENT);
        return;
    }
    double* count = A.count + q.k0;
    double* percent = A.percent + q.k0;
    double* prior = W.prior + q.k0;
    const unsigned char* filter = A.filter + q.k0;
    const int k = A.def_key[q.d0 + W.trial[q.d0 + b]];
    const int accepted = st.accepted, has_prior = st.has_prior;
    const double total = filter[k] ? W.ttotal[q.d0 + b] : st.total;
    __syncthreads();
    if (tid == 0) {
        if (accepted < A.accepted_cap) A.accepted_key[(long long)p * A.accepted_cap + accepted] = k;
        else A.overflow[p] |= FSQ_BACKGROUND_OVERFLOW_ACCEPTED;
        count[k] = W.interp[q.d0 + b];
        st.accepted = accepted + 1;
    }
    __syncthreads();
    if (has_prior) {                                               // max(abs_diffs) < 0.001 (:6007-6010)
        int moved = 0;
        for (int j = tid; j < q.N; j += THREADS) {
            const double d = fabs(count[j] - prior[j]);
            moved |= (d >= 0.001) || (j == 0 && d != d);
        }
        if (!__syncthreads_or(moved)) {
            finish(A, W, q, p, FSQ_BACKGROUND_CONVERGED);
            return;
        }
    }
    for (int j = tid; j < q.N; j += THREADS) {
        const double c = count[j];
        prior[j] = c;
        percent[j] = filter[j] ? c / total : 0.0;
    }
    if (tid == 0) {
        st.has_prior = 1;
        st.total = total;
    }
    __syncthreads();                                               // (the percents are the workgroup's)
    list_trials(A, W, q, p, s_rv, s_ri, s_wcnt);
}

bool sizes_ok(int32_t P, int64_t N, int64_t D, int64_t nb)
{
    return P >= 0 && P <= 65535 && N >= 0 && N < (1ll << 31) && D >= 0 && D < (1ll << 31) && nb >= 0 && nb < (1ll << 31);
}

int64_t up8(int64_t x) { return (x + 7) & ~(int64_t)7; }

}  // namespace

extern "C" int64_t fsq_background_workspace_bytes(int32_t P, int64_t N, int64_t D, int64_t nb)
{
    if (!sizes_ok(P, N, D, nb)) return FSQ_EINVAL;
    return up8((int64_t)P * (int64_t)sizeof(State)) + up8((int64_t)P * 4) + up8(N * 4) + up8(nb * 4) + 2 * N * 8 + 4 * D * 8 + up8(D * 4) + 8;
}

extern "C" int fsq_background_iterate(const FsqBackgroundArgs* args, void* ws, int64_t ws_bytes, void* stream_)
{
    if (!args) return FSQ_EINVAL;
    const FsqBackgroundArgs& A = *args;
    const int P = A.n_problems;
    const int64_t N = A.n_keys, D = A.n_defined;
    if (!sizes_ok(P, N, D, A.n_neighbours) || A.n_first < 0 || A.n_rest < 0 || A.max_iterations < 0 || A.accepted_cap < 0 ||
        A.undefined_cap < 0 || A.max_defined < 0 || A.max_defined > D)
        return FSQ_EINVAL;
    if (P == 0) return FSQ_OK;
    if (!A.key_off || !A.def_off || !A.first_off || !A.rest_off || !A.num_cycles || !A.include_multidrop || !A.sigma_threshold ||
        !A.nb_off || !A.stop_reason || !A.n_passes || !A.n_accepted || !A.overflow)
        return FSQ_EINVAL;
    if (N > 0 && (!A.code || !A.sorted_code || !A.sorted_index || !A.filter || !A.count || !A.percent || !A.rounded)) return FSQ_EINVAL;
    if (D > 0 && (!A.def_key || !A.def_avg || !A.def_std)) return FSQ_EINVAL;
    if ((A.n_first > 0 && !A.und_first) || (A.n_rest > 0 && !A.und_rest) || (A.accepted_cap > 0 && !A.accepted_key)) return FSQ_EINVAL;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < fsq_background_workspace_bytes(P, N, D, A.n_neighbours)) return FSQ_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    Work W;
    char* at = (char*)ws;
    const int64_t head_bytes = up8((int64_t)P * (int64_t)sizeof(State)) + up8((int64_t)P * 4);
    W.state = (State*)at;      at += up8((int64_t)P * (int64_t)sizeof(State));
    W.done = (int*)at;         at += up8((int64_t)P * 4);
    W.nb_cnt = (int*)at;       at += up8(N * 4);
    W.nb = (int*)at;           at += up8(A.n_neighbours * 4);
    W.prefix = (double*)at;    at += N * 8;
    W.prior = (double*)at;     at += N * 8;
    W.z = (double*)at;         at += D * 8;
    W.interp = (double*)at;    at += D * 8;
    W.diff = (double*)at;      at += D * 8;
    W.ttotal = (double*)at;    at += D * 8;
    W.trial = (int*)at;
    FSQ_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)head_bytes, stream));
    FSQ_HIP_CHECK(hipMemsetAsync(A.overflow, 0, (size_t)P * sizeof(int32_t), stream));
    if (N > 0) {
        hipLaunchKernelGGL(kbg_neighbours, dim3((unsigned)((N + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, A, W);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(kbg_first, dim3((unsigned)P), dim3(THREADS), 0, stream, A, W);
    FSQ_HIP_CHECK(hipGetLastError());
    const unsigned trial_blocks = (unsigned)((A.max_defined + TRIAL_THREADS - 1) / TRIAL_THREADS);
    std::vector<int> done((size_t)P, 0);
    // every batch advances every running problem by FSQ_BACKGROUND_BATCH_PASSES passes, and the pass after max_iterations stops it
    const int64_t batches = (int64_t)A.max_iterations / FSQ_BACKGROUND_BATCH_PASSES + 2;
    for (int64_t batch = 0; batch < batches; batch++) {
        for (int pass = 0; pass < FSQ_BACKGROUND_BATCH_PASSES; pass++) {
            hipLaunchKernelGGL(kbg_head, dim3((unsigned)P), dim3(THREADS), 0, stream, A, W);
            if (trial_blocks > 0) hipLaunchKernelGGL(kbg_trials, dim3(trial_blocks, (unsigned)P), dim3(TRIAL_THREADS), 0, stream, A, W);
            hipLaunchKernelGGL(kbg_tail, dim3((unsigned)P), dim3(THREADS), 0, stream, A, W);
        }
        FSQ_HIP_CHECK(hipGetLastError());
        FSQ_HIP_CHECK(hipMemcpyAsync(done.data(), W.done, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, stream));
        FSQ_HIP_CHECK(hipStreamSynchronize(stream));
        bool all = true;
        for (int p = 0; p < P; p++) all = all && done[(size_t)p] != 0;
        if (all) return FSQ_OK;
    }
    return FSQ_EINTERNAL;
}
