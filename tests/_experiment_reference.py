"""NumPy restatement of the two glue kernels of include/fsq_experiment.h (no GPU, no package code beyond the record layout):
what tests/test_experiment_host.py pins to the reference's recorded output and tests/test_gpu_experiment.py compares the
kernels with."""
import numpy as np

STATUS_OK, STATUS_REKEY_ASSERT, STATUS_INVALID = 0, 1, 2
REC_H0, REC_W0, REC_KEY_H, REC_KEY_W = 0, 8, 120, 124          # byte offsets inside a 378- or 428-byte peak record


def spot_accepted(h, w, h_0, w_0, H, W, size=5):
    """Does Spot.__init__ (reference flexlibrary.py:98-121) take a Spot at (h, w) whose fit is centred at (h_0, w_0)?  As
    Python's operator precedence reads the reference's test: refused iff the window leaves the image and
    (not (r <= h_0 < H - r)) and (r <= w_0 < W - r)."""
    r = (size - 1) // 2
    if 0 <= h - r and h + r < H and 0 <= w - r and w + r < W:
        return True
    return not ((not (r <= h_0 < H - r)) and (r <= w_0 < W - r))


def record_fields(records):
    """uint8 [k, 378 | 428] -> (h_0, w_0 float64 [k], key_h, key_w int32 [k]), read byte-wise (the records are unaligned)."""
    rec = np.ascontiguousarray(records, dtype=np.uint8)
    rec = rec.reshape(-1, rec.shape[-1]) if rec.ndim == 2 else rec.reshape(0, 378)

    def col(off, dtype, n):
        return np.ascontiguousarray(rec[:, off:off + n]).view(dtype).reshape(-1)
    return col(REC_H0, "<f8", 8), col(REC_W0, "<f8", 8), col(REC_KEY_H, "<i4", 4), col(REC_KEY_W, "<i4", 4)


def spot_table(records, peaks, H, W, spot_size=5):
    """fsq_experiment_spot_table: -> dict(hw int32 [k', 2], spot_record int32 [k'], counts, discarded, status int32 [n_frames])."""
    h_0, w_0, key_h, key_w = record_fields(records)
    n_records = len(h_0)
    peaks = np.asarray(peaks, dtype=np.int64).reshape(-1)
    n = len(peaks)
    counts, discarded, status = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    hw, spot_record = [], []
    a = 0
    for f, p in enumerate(peaks.tolist()):
        if p == -1:
            status[f] = STATUS_REKEY_ASSERT
            continue
        if p < -1 or a + p > n_records:
            status[f] = STATUS_INVALID
            a += max(p, 0)                       # (the frame's claim still moves the frames after it)
            continue
        for rec in range(a, a + p):
            if spot_accepted(int(key_h[rec]), int(key_w[rec]), float(h_0[rec]), float(w_0[rec]), H, W, spot_size):
                hw.append((int(key_h[rec]), int(key_w[rec])))
                spot_record.append(rec)
                counts[f] += 1
            else:
                discarded[f] += 1
        a += p
    return {"hw": np.array(hw, np.int32).reshape(-1, 2), "spot_record": np.array(spot_record, np.int32), "counts": counts,
            "discarded": discarded, "status": status}


def trace_rows(traces, n_traces, field_start, hw, n_frames):
    """fsq_experiment_trace_rows (with fsq_experiment_trace_starts): traces int32 [total, F] as fsq_greedy_tracking leaves
    them -> dict(trace_hw int32 [N, F, 2], trace_spot int32 [N, F], trace_seq int32 [N], seq_start int32 [n_seq + 1])."""
    F = int(n_frames)
    traces = np.asarray(traces, dtype=np.int64).reshape(-1, F)
    hw = np.asarray(hw, dtype=np.int32).reshape(-1, 2)
    nt = np.maximum(np.asarray(n_traces, dtype=np.int64).reshape(-1), 0)
    fs = np.asarray(field_start, dtype=np.int64).reshape(-1)
    seq_start = np.concatenate([[0], np.cumsum(nt)]).astype(np.int32)
    N = int(seq_start[-1])
    t_hw = np.full((N, F, 2), -1, np.int32)
    t_spot = np.full((N, F), -1, np.int32)
    t_seq = np.zeros(N, np.int32)
    for s in range(len(nt)):
        first, end = int(fs[s]), int(fs[s + 1])
        for i in range(int(nt[s])):
            n, row = int(seq_start[s]) + i, first + i
            t_seq[n] = s
            if row >= end:
                continue
            for f in range(F):
                spot = int(traces[row, f])
                if spot >= 0 and first + spot < end:
                    t_spot[n, f] = first + spot
                    t_hw[n, f] = hw[first + spot]
    return {"trace_hw": t_hw, "trace_spot": t_spot, "trace_seq": t_seq, "seq_start": seq_start}

