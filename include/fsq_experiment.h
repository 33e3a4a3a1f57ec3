/* fsq_experiment.h - C ABI of the glue that keeps a sequence experiment on the device (libfsq_hip.so, gfx950).
 *
 * The reference's basic_experiment_script fits every cycle's image, loads the fits as Spots, registers consecutive cycles,
 * tracks the Spots and reduces the tracks.  fsq_find_peptides, fsq_phase_correlate, fsq_greedy_tracking (include/fsq.h),
 * fsq_sequence_photometry and fsq_sequence_category_counts (include/fsq_sequence.h) are the stages; the two entries here turn
 * the output of one stage into the input of the next, so that no Python object per Spot is made in between:
 *
 *   fsq_experiment_spot_table   peak records -> the (h, w) tables fsq_greedy_tracking reads: the loop of
 *                               Experiment.easy_load_processed_image (flexlibrary.py:549-563) with the acceptance test of
 *                               Spot.__init__ (:98-121)
 *   fsq_experiment_trace_rows   fsq_greedy_tracking's traces -> the rows fsq_sequence_photometry reads
 *
 * One *sequence* is one field of one channel; a *frame* is one image of a sequence.  Conventions are those of
 * include/fsq_sequence.h: every entry enqueues on `stream` and does not synchronise, buffers are the caller's, per-item
 * status goes to device arrays, return codes are those of include/fsq.h. */
#ifndef FSQ_EXPERIMENT_H
#define FSQ_EXPERIMENT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d_status of fsq_experiment_spot_table, one word per frame */
#define FSQ_EXPERIMENT_OK 0
#define FSQ_EXPERIMENT_REKEY_ASSERT 1       /* the frame's peak count is -1: the re-key assertion of pflib.py:518 fired */
#define FSQ_EXPERIMENT_INVALID 2            /* a peak count below -1, or the frame's records reach beyond n_records */

/* Bytes of device workspace fsq_experiment_spot_table needs; -1 for invalid sizes. */
int64_t fsq_experiment_spot_table_workspace_bytes(int64_t n_records, int32_t n_frames);

/* Peak records -> Spot tables.
 *   d_records     uint8 [n_records][record_bytes]  the byte table fsq_find_peptides leaves (record_bytes 378, or 428 for
 *                 FSQ_PIXELS_U32 frames): all frames in order.  A record's fields are only 2-byte aligned; they are read
 *                 16 bits at a time.  Read: h_0, w_0 (double, bytes 0 and 8) and key_h, key_w (int32, bytes 120 and 124).
 *   d_peaks       int32 [n_frames]  records per frame; -1: the frame failed and owns no records
 *   H, W          frame shape;  spot_size  odd size of a Spot (5 for every fit of the reference), r = (spot_size - 1) / 2
 * A record becomes a Spot at (h, w) = (key_h, key_w) unless Spot.__init__ raises for it:
 *   the window leaves the image, not (0 <= h - r and h + r < H and 0 <= w - r and w + r < W),
 *   AND (not (r <= h_0 < H - r)) and (r <= w_0 < W - r)
 * - the reference's test as Python's operator precedence reads it: a window that leaves the image through the rows alone is
 * refused, one that leaves it through the columns (a corner included) is kept.
 * Outputs (accepted Spots keep record order: frame after frame, inside a frame in the order of its records):
 *   d_hw          int32 [n_records][2]  (h, w) of the Spots, compacted: the first *d_n_spots rows are written
 *   d_spot_record int32 [n_records]     record index of every Spot
 *   d_counts      int32 [n_frames]      Spots per frame
 *   d_discarded   int32 [n_frames]      records per frame that Spot.__init__ refused
 *   d_status      int32 [n_frames]      FSQ_EXPERIMENT_*; a frame that is not OK has counts = discarded = 0
 *   d_n_spots     int32 [1]             sum of d_counts
 * n_records < 2^31.  n_frames == 0 writes *d_n_spots = 0 and nothing else. */
int fsq_experiment_spot_table(const uint8_t* d_records, int64_t n_records, int32_t record_bytes, const int32_t* d_peaks,
                              int32_t n_frames, int32_t H, int32_t W, int32_t spot_size, int32_t* d_hw, int32_t* d_spot_record,
                              int32_t* d_counts, int32_t* d_discarded, int32_t* d_status, int32_t* d_n_spots, void* d_ws,
                              int64_t ws_bytes, void* stream);

/* Exclusive scan of the traces per sequence: d_seq_start[s] = sum of max(d_n_traces[0 .. s-1], 0), [n_seq] = N, the number of
 * rows fsq_experiment_trace_rows writes.  The caller reads that one word back to size the outputs. */
int fsq_experiment_trace_starts(const int32_t* d_n_traces, int32_t n_seq, int32_t* d_seq_start, void* stream);

/* fsq_greedy_tracking's output -> fsq_sequence_photometry's input; traces stay in tracking order, sequences ascending.
 *   d_traces      int32 [total][n_frames]  as fsq_greedy_tracking leaves it: sequence s owns rows d_field_start[s] ..
 *                 + n_traces[s] - 1; an entry is a spot number counted from the sequence's first spot, or -1
 *   d_seq_start   int32 [n_seq + 1]  from fsq_experiment_trace_starts (n_traces = the differences); N = d_seq_start[n_seq]
 *   d_field_start int32 [n_seq + 1]  first spot of every sequence in d_hw; [n_seq] = total
 *   d_hw          int32 [total][2]   the Spot table
 *   n_rows        the N the outputs were sized for; rows beyond it are not written
 * Outputs:
 *   d_trace_hw    int32 [N][n_frames][2]  (h, w) of the trace's Spot, (-1, -1) where it has none
 *   d_trace_spot  int32 [N][n_frames]     row of that Spot in d_hw, -1 where there is none
 *   d_trace_seq   int32 [N]               sequence of every trace
 * A trace row or spot number outside its sequence's part of the tables reads as "no Spot". */
int fsq_experiment_trace_rows(const int32_t* d_traces, const int32_t* d_seq_start, const int32_t* d_field_start,
                              const int32_t* d_hw, int32_t n_seq, int32_t n_frames, int64_t n_rows, int32_t* d_trace_hw,
                              int32_t* d_trace_spot, int32_t* d_trace_seq, void* stream);

#ifdef __cplusplus
}
#endif
#endif
