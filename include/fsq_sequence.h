/* fsq_sequence.h - C ABI of the sequence-experiment reduction (libfsq_hip.so, gfx950).
 *
 * The step of the reference's basic_experiment_script after tracking: every track of every field and channel is
 * reduced to an ON/OFF pattern and a photometry per frame (SequenceExperiment.fill_in_trace / interpolate_spots,
 * flexlibrary.py:1842-2032; discard_invalid_traces :2034-2063; binary_trace_categories_photometry :2065-2129), and
 * the patterns are counted per sequence (count_binary_trace_categories).  One *sequence* is one field of one channel.
 * Every entry enqueues on `stream` and does not synchronise.  Return codes are those of include/fsq.h. */
#ifndef FSQ_SEQUENCE_H
#define FSQ_SEQUENCE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_SEQUENCE_MAX_FRAMES 64          /* the category is one bit per frame; more frames: FSQ_ENOTIMPL */

#define FSQ_SEQUENCE_MEXICAN_HAT 0          /* Spot.mexican_hat_photometry_metric, as fsq_mexican_hat of include/fsq.h */
#define FSQ_SEQUENCE_SIMPLE 1               /* Spot.simple_photometry_metric: sum of the clipped spot_size^2 window */

/* bits of d_flags */
#define FSQ_SEQUENCE_DETECTED 1             /* the trace holds a detected Spot in this frame */
#define FSQ_SEQUENCE_INTERPOLATED 2         /* the Spot was made by interpolate_spots */
#define FSQ_SEQUENCE_WINDOW_INSIDE 4        /* Spot.valid_slice: the photometry window lies fully inside the frame */

/* Bytes of device workspace fsq_sequence_photometry needs (the accumulated offsets of every sequence). */
int64_t fsq_sequence_workspace_bytes(int32_t n_seq, int32_t n_frames);

/* For every (trace, frame): where the Spot is, whether it counts, and its photometry.
 *   d_frames     uint16 [n_seq][n_frames][H][W] (the _u32 entry: uint32, values < 2^31)
 *   d_trace_hw   int32  [n_traces][n_frames][2]   (h, w) of the detected Spot; a negative h or w: no Spot in that frame
 *   d_trace_seq  int32  [n_traces]                sequence of the trace (outside [0, n_seq): every output of the trace
 *                                                 reads "no Spot", d_trace_valid 0)
 *   d_offsets    double [n_seq][n_frames][2]      (d_h, d_w) of every frame relative to the one before; [0] is (0, 0)
 *   radius, brim_size                             the hat's window radius and brim width (FSQ_SEQUENCE_MEXICAN_HAT)
 *   spot_size    odd size of a Spot: an interpolated Spot exists iff r <= h < H - r and r <= w < W - r with
 *                r = (spot_size - 1) / 2; the window of FSQ_SEQUENCE_SIMPLE
 *   interpolate  0: an undetected frame has no Spot; 1: it is filled in by fill_in_trace
 * Outputs:
 *   d_hw         int32  [n_traces][n_frames][2]   position used, (-1, -1) = None
 *   d_phot       double [n_traces][n_frames]      photometry, NaN where None
 *   d_flags      uint8  [n_traces][n_frames]      FSQ_SEQUENCE_* bits
 *   d_category   uint64 [n_traces]                bit f = detected in frame f
 *   d_trace_valid uint8 [n_traces]                1: every frame holds a Spot and every window lies inside the frame (the rule
 *                                                 of discard_invalid_traces when interpolate = 1)
 * All sequences of one call share n_frames, H, W. */
int fsq_sequence_photometry(const uint16_t* d_frames, int32_t n_seq, int32_t n_frames, int32_t H, int32_t W,
                            const int32_t* d_trace_hw, const int32_t* d_trace_seq, int64_t n_traces, const double* d_offsets,
                            int32_t radius, int32_t brim_size, int32_t spot_size, int32_t method, int32_t interpolate,
                            int32_t* d_hw, double* d_phot, uint8_t* d_flags, uint64_t* d_category, uint8_t* d_trace_valid,
                            void* d_ws, int64_t ws_bytes, void* stream);
int fsq_sequence_photometry_u32(const uint32_t* d_frames, int32_t n_seq, int32_t n_frames, int32_t H, int32_t W,
                                const int32_t* d_trace_hw, const int32_t* d_trace_seq, int64_t n_traces, const double* d_offsets,
                                int32_t radius, int32_t brim_size, int32_t spot_size, int32_t method, int32_t interpolate,
                                int32_t* d_hw, double* d_phot, uint8_t* d_flags, uint64_t* d_category, uint8_t* d_trace_valid,
                                void* d_ws, int64_t ws_bytes, void* stream);

/* Bytes of device workspace fsq_sequence_category_counts needs for n_traces traces. */
int64_t fsq_sequence_category_counts_workspace_bytes(int64_t n_traces);

/* Counts of traces per (sequence, pattern): a flat table of *d_n_groups rows (at most n_traces) in no particular order.
 *   d_category, d_trace_seq   as above; d_select uint8 [n_traces] or NULL: only traces with a non-zero entry are counted
 *   d_group_seq int32, d_group_pattern uint64, d_group_count int32, d_group_first int32 [n_traces]: sequence, pattern,
 *   number of traces and the smallest trace index of every group; d_n_groups int32 [1]. */
int fsq_sequence_category_counts(const uint64_t* d_category, const int32_t* d_trace_seq, const uint8_t* d_select,
                                 int64_t n_traces, int32_t* d_group_seq, uint64_t* d_group_pattern, int32_t* d_group_count,
                                 int32_t* d_group_first, int32_t* d_n_groups, void* d_ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
