/*
 * sslrec_hip.h -- C ABI of libsslrec_hip.so, the MI355X (gfx950) implementation of
 * SSLRec's general-CF hot path.
 *
 * The reference (HKUDS/SSLRec) is pure Python and has NO FFI of its own: the path is a
 * sequence of PyTorch calls.  Each entry point below replaces one such call sequence;
 * the reference file:line it stands in for is cited on every declaration (paths are
 * relative to the reference root).  INTEGRATION.md shows the ctypes binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - nothing is allocated inside: the caller owns every buffer (workspace sizes come
 *     from the *_ws_bytes queries);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronizes;
 *   - return value is a hipError_t cast to int (0 = hipSuccess); argument errors
 *     return SSLREC_E_BADARG without launching anything;
 *   - all arithmetic is fp32; row indices into embedding tables are int64 (what
 *     trainer/trainer.py:64 puts on the device), graph indices are int32.
 */
#ifndef SSLREC_HIP_H
#define SSLREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSLREC_ABI_VERSION 7
#define SSLREC_E_BADARG 1001   /* distinct from any hipError_t */

int sslrec_abi_version(void);

/* bits[0 .. ceil(n_rows / 32)) = the set { idx0[i] + off0, idx1[i] + off1, idx2[i] + off2 : i < n } as a bitmap (idx1 / idx2 nullable);
 * n_rows <= 1,048,576 (one workgroup builds it in LDS).  The rows a fused BPR backward (sslrec_bpr_bwd_f32) writes of a stacked
 * [users; items] gradient table: anchors at offset 0, positives and negatives at offset n_user (lightgcn.py:49-52). */
int sslrec_row_bits3(const int64_t *idx0, int64_t off0, const int64_t *idx1, int64_t off1, const int64_t *idx2, int64_t off2,
                     int32_t n, int32_t n_rows, uint32_t *bits, void *stream);

/* ------------------------------------------------------------------------------------
 * Sparse propagation  Y = A * X      (replaces torch.spmm(adj, embeds),
 * models/general_cf/lightgcn.py:28-29; its autograd backward dX = A^T dY,
 * trainer/trainer.py:67; and LightGCL's gather/index_add_ product,
 * models/general_cf/lightgcl.py:58-65)
 *
 * A is held in a STREAMED, PACKED CSR built for ONE embedding size d.  Rows keep their
 * entries sorted by column (the summation order); rows longer than a cap are cut into chunks;
 * the row segments are dealt to `n_waves` work streams of (nearly) equal length -- 32 per
 * compute unit, one per resident wavefront.  A stream is a sequence of SLOTS: G = 256/d
 * consecutive slots form one vector LOAD (one 16-byte read per lane fetches G neighbour rows of
 * 4*d bytes each; slot k belongs to lane group k % G), every row segment occupies whole loads
 * (padded with col = -1, val = 0), 4 loads form a block and a block is stored group-major:
 *     element(k) = (k / 4G) * 4G + (k % G) * 4 + (k / G) % 4
 * so that a lane reads the 4 columns (values) it needs for a block with one 16-byte load.
 * Chunk partial sums go to a scratch slab and are combined in slot order by a second small
 * kernel (no atomics, bit-deterministic).
 * ---------------------------------------------------------------------------------- */
typedef struct sslrec_csr {
    int32_t n_rows, n_cols, nnz;   /* nnz = real entries (pads excluded)                   */
    int32_t d;                     /* embedding size the layout was packed for             */
    int32_t n_elem;                /* elements of col[] / val[] (pads included)            */
    const int32_t *col;        /* [n_elem] column of each slot, -1 = pad                  */
    const float   *val;        /* [n_elem]                                                */
    int32_t n_waves;           /* number of work streams                                  */
    const int32_t *w_start;    /* [n_waves]   first element of stream w (multiple of 4G)  */
    const int32_t *w_len;      /* [n_waves]   LOADS in stream w                           */
    const int32_t *r_ptr;      /* [n_waves+1] row segments of stream w = [r_ptr[w], r_ptr[w+1]) */
    int32_t n_rseg;
    const int32_t *r_len;      /* [n_rseg] LOADS of each row segment, in stream order     */
    const int32_t *r_dst;      /* [n_rseg] >=0: output row; <0: partial slot ~x           */
    int32_t n_long;            /* rows that were cut into chunks                          */
    const int32_t *long_row;   /* [n_long]                                                */
    const int32_t *long_ptr;   /* [n_long+1] slots of row i = [long_ptr[i],long_ptr[i+1]) */
    int32_t n_slots;           /* partial slab holds n_slots*d floats                     */
} sslrec_csr_t;                /* the struct itself lives in HOST memory                  */

/* ZERO-VALUED ENTRIES.  Pads carry the value 0 and an edge-dropped view of the streamed / row-bundled layouts may zero an
 * entry's value instead of removing it: there an element whose stored value is exactly 0 contributes NOTHING, even when the row it
 * points at holds Inf / NaN (a pad reads row 0).  The column-swept kernel removes dropped entries from its streams and marks pads by
 * their packed word (-1), so it has no such rule: an explicit zero-weight edge of the INPUT matrix is multiplied like any other
 * (0 * Inf = NaN, as torch.spmm gives).  The layouts therefore differ only on explicit zeros in the caller's value array whose
 * source row is non-finite -- the reference's adjacencies hold none (every value is 1 / sqrt(d_i d_j) > 0). */
/* Optional fused epilogue applied to each finished output row y (all pointers nullable):
 *   noise  : y += eps * sign(y) * noise_row / max(||noise_row||_2, 1e-12)
 *            (EmbedPerturb, models/aug_utils.py:125-132; noise is the caller's draw)
 *   acc_in/acc_out : acc_out_row = acc_in_row + y   (the layer SUM of lightgcn.py:41 in
 *            forward; the "+G" of the backward recurrence).  acc_in may equal acc_out. */
typedef struct sslrec_epilogue {
    const float *noise; float eps;
    const float *acc_in; float *acc_out;
    /* device-side noise (perf mode): with noise == NULL and philox != NULL the uniform noise row
     * is COMPUTED in the epilogue (Philox4x32-10, see "device-side augmentation RNG" below): no N x d tensor exists */
    const uint64_t *philox; uint32_t philox_stream;
    /* EmbedPerturb when the launch works on a COLUMN SLICE of the table (feature-sliced tables, sslrec_amd/feature_shard.py:
     * a GPU holds d/P columns of every row, but the perturbation's norm runs over the FULL row of the reference's [N, d] draw):
     *   noise_sumsq [n_rows] (nullable): squared L2 norm of the full noise row -- replaces the norm over the launch's own columns
     *                (supplied noise: the ranks all-reduce their partial sums of squares; Philox noise: every rank computes all d
     *                columns' draws of a row, sslrec_philox_row_sumsq);
     *   noise_row_stride / noise_col_off (floats, multiples of 4; 0 / 0 = the launch's own table): position of this launch's
     *                columns inside the full noise row -- the Philox element index of a computed draw is taken in the FULL table,
     *                so a slice of the result equals the same columns of the one-GPU result. */
    const float *noise_sumsq; int32_t noise_row_stride, noise_col_off;
    /* acc_out_row += axpy_alpha * (axpy_scale ? *axpy_scale : 1) * axpy_x_row (nullable; needs acc_out): the regularizer's gradient
     * 2 * reg_weight * g * E0 (loss_utils.py:20-24) folded into the LAST product of the backward recurrence instead of a pass of
     * its own over the table plus an elementwise add */
    const float *axpy_x; float axpy_alpha; const float *axpy_scale;
    /* HINT (nullable): x_row_bits[r / 32] bit (r % 32) clear = row r of X is all zeros.  The column-swept kernel then treats the
     * entries of that column like pads (no gather of the row, no accumulate); the other kernels ignore the hint.  The result is the
     * dense product's (x + 0 = x; a zero's sign aside).  Use: the first product of the backward recurrence when the incoming gradient
     * is the BPR loss's -- it touches <= 3B of the N rows (sslrec_row_bits3 builds the bitmap from the batch's indices). */
    const uint32_t *x_row_bits;
    /* DEFERRED layer sum (n_sum_in <= SSLREC_MAX_SUM_IN; needs acc_in and acc_out): acc_out_row = (((acc_in_row + sum_in[0]_row) + ...)
     * + sum_in[n-1]_row) + y.  The forward layer loop (lightgcn.py:38-41) then writes only Y in the launches l < L and the LAST launch
     * forms E0 + E1 + ... + E_L -- added in layer order, so the result has the bits of the running sum -- instead of every launch
     * reading and writing the running sum: 2 (L - 1) n_rows d 4 fewer bytes written per forward.  Column-swept kernel on layouts for
     * which sslrec_swept_deferred_sum_ok() returns 1 only (elsewhere n_sum_in != 0 is SSLREC_E_BADARG and the caller keeps the
     * running sum). */
    int32_t n_sum_in; const float *sum_in[3];
    /* FACTORIZED normalization (ABI 6; column-swept kernel only, elsewhere scale_flags != 0 is SSLREC_E_BADARG).  The reference's
     * adjacency is D^-1/2 A D^-1/2 with a 0/1 matrix A (data_handler_general_cf.py:37-51, binarized at :65), LightGCL's is
     * 1/sqrt(d_u d_i) (lightgcl.py:17-20): value(i, j) = r[i] * c[j].  So a layer chain (lightgcn.py:38-41) can carry the SCALED table
     * F_l = c (.) E_l as the gathered operand and never read the value stream:
     *   SSLREC_SCALE_PATTERN : every entry counts 1 -- the value array is not read; the row sum s of the gathered rows becomes the
     *                          product's row y = row_scale[row] * s before any other epilogue (noise, layer sum);
     *   SSLREC_SCALE_Y       : Y receives row_scale[row] * y (the next pattern launch's operand) -- acc_out still adds the plain y;
     *   SSLREC_SCALE_ACC     : acc_out receives row_scale[row] * (acc_in + y [+ axpy]) (the backward recurrence g <- G + A^T g carried
     *                          as c (.) g).
     * row_scale [n_rows] is needed by all three.  A chain = one valued launch with SCALE_Y (its operand E_0 is unscaled), then pattern
     * launches.  The products agree with the valued ones to rounding (r[i] * c[j] is rounded once more in the value array), not
     * bit for bit. */
    const float *row_scale; int32_t scale_flags;
} sslrec_epilogue_t;           /* host memory */
#define SSLREC_MAX_SUM_IN 3
#define SSLREC_SCALE_PATTERN 1
#define SSLREC_SCALE_Y 2
#define SSLREC_SCALE_ACC 4

/* d must be 32, 64, 128 or 256 and equal A->d.  Y may be NULL when only acc_out is wanted.
 * col/val/r_len/w_len default to A's arrays when the override pointers are NULL; the
 * overrides are how an edge-dropped or re-valued view (below) is multiplied (r_len and
 * w_len overrides come as a pair).
 * partial_ws: >= A->n_slots*d floats (may be NULL when n_slots==0). */
int sslrec_spmm_csr_f32(const sslrec_csr_t *A,
                        const int32_t *col_override, const float *val_override,
                        const int32_t *r_len_override, const int32_t *w_len_override,
                        const float *X, int32_t d, float *Y,
                        const sslrec_epilogue_t *epi, float *partial_ws, void *stream);

/* NARROW tables beyond the column-swept layout -- d = 8 or 16 (a GPU's d/P columns of every row under feature slicing,
 * sslrec_amd/feature_shard.py; BASELINE config 5: 10 M-row tables, 128 / 8 = 16 columns) and optionally 32: the ROW-BUNDLED
 * streamed layout.  Replaces the same reference call (lightgcn.py:28-29 / lightgcl.py:58-65).  At these widths one
 * 16-byte-per-lane wave instruction gathers G = 256/d = 32 / 16 / 8 neighbour rows, so every lane group (d/4 lanes) owns a
 * whole OUTPUT row and keeps its sum in registers: no cross-lane reduction, no LDS, control stays wave-uniform.  Row
 * segments (a row, or a chunk of a row longer than the cap: partial sums to the slab, combined in slot order by the
 * long-row kernel) are sorted by length and G consecutive ones form a BUNDLE that runs for the longest member's steps
 * (rounded up to S = d/4 steps; shorter members are padded with col = -1: 2-5 % pads on power-law graphs of mean degree 32);
 * bundles are dealt (longest-processing-time-first) to n_waves streams.  A stream is stored like a column-swept stream:
 * 64-dword blocks of S steps, dword g*(64/G) + j of a block = the entry of (step j, lane group g), so ONE coalesced dword
 * load per array fetches S steps for all G rows and a DPP quad / row permute hands every lane its entry.
 *   col/val [n_elem]; w_ptr [n_waves+1] bundles of stream w (stored back to back from element w_start[w]);
 *   b_steps [n_bundles] steps of a bundle (multiple of S, may be 0: rows without entries are written as zeros);
 *   b_dst [n_bundles * G]: output row of lane group g (>= 0), partial slot ~x (< 0), or SSLREC_BUNDLE_NONE. */
#define SSLREC_BUNDLE_NONE (-2147483647 - 1)
typedef struct sslrec_bundled {
    int32_t n_rows, n_cols, nnz, d;
    int32_t n_elem;
    const int32_t *col; const float *val;
    int32_t n_waves;
    const int32_t *w_start;    /* [n_waves]   first element of stream w (multiple of 64)            */
    const int32_t *w_ptr;      /* [n_waves+1]                                                       */
    int32_t n_bundles;
    const int32_t *b_steps;    /* [n_bundles]                                                       */
    const int32_t *b_dst;      /* [n_bundles * 256/d]                                               */
    int32_t n_long;
    const int32_t *long_row, *long_ptr;
    int32_t n_slots;
} sslrec_bundled_t;            /* host memory; arrays on the device */

/* val_override / b_steps_override (nullable): a re-valued view / a view whose bundles were shortened.  d must equal A->d.
 * partial_ws: >= A->n_slots * d floats (NULL when n_slots == 0). */
int sslrec_spmm_bundled_f32(const sslrec_bundled_t *A, const float *val_override, const float *X, int32_t d, float *Y,
                            const sslrec_epilogue_t *epi, float *partial_ws, void *stream);
/* the same product over a VIEW of the layout: col / val / b_steps / w_blocks overrides (all nullable; b_steps and w_blocks together, with
 * col: a compacted edge-dropped view, sslrec_bundled_compact) */
int sslrec_spmm_bundled_view_f32(const sslrec_bundled_t *A, const int32_t *col_override, const float *val_override,
                                 const int32_t *b_steps_override, const int32_t *w_blocks_override, const float *X, int32_t d, float *Y,
                                 const sslrec_epilogue_t *epi, float *partial_ws, void *stream);

/* Column-swept variant of the same product for output tables that fit the chip's LDS
 * (n_rows * d * 4 <= n_blocks * SSLREC_SWEPT_LDS_BYTES; amazon-book at d=64: 36.9 MB of 40 MB).
 * Replaces the same reference call (lightgcn.py:28-29) with the same epilogue.  One workgroup per CU
 * owns `n_slots` LDS accumulators (a slot = an output row, or one interleaved chunk of a heavy row);
 * its 16 waves x (256/d) lane groups own disjoint slots and walk their edges sorted by column, so the
 * CUs of an XCD sweep X together (sslrec_amd/csrc/spmm_swept.hip).
 *   pack/val [n_elem]: per wave a stream of 64-dword blocks of S = min(16, 64/G) steps, G = 256/d
 *                      lane groups: dword g*(64/G) + j of a block = the entry of (step j, lane group g), repeated in every
 *                      16-lane row of the lane group at d >= 128 (one coalesced dword load per array fetches S steps, a DPP
 *                      broadcast hands every lane its entry); pack = column (low 20 bits) | slot << 20, -1 = pad;
 *                      w_start [16*n_blocks] element offsets, w_steps steps (multiples of S)
 *   flush records (f_row global row, f_start first slot, f_n slots to add): a row that occupies ONE slot belongs to one
 *                      lane group, hence to one wave, which writes it out as soon as its own sweep is over (no barrier; the
 *                      stores overlap the slower waves' gathers): records [wf_ptr[w], wf_ptr[w+1]) of wave w = 16*block + wave;
 *                      rows cut into chunks are added up by the whole block after its barrier: records [cf_ptr[b], cf_ptr[b+1])
 * d (= A->d) is 32, 64, 128 or 256, or -- for FEATURE-SLICED tables, where a GPU holds d/P columns of every row
 * (sslrec_amd/feature_shard.py) -- 16 or 8 (beyond this layout's size limits those run on the row-bundled layout above). */
#define SSLREC_SWEPT_LDS_BYTES 163840
typedef struct sslrec_swept {
    int32_t n_rows, n_cols, nnz, d;
    int32_t n_elem, n_blocks, n_slots;
    const int32_t *pack; const float *val;
    const int32_t *w_start, *w_steps;
    const int32_t *wf_ptr;                 /* [16*n_blocks+1] */
    const int32_t *cf_ptr;                 /* [n_blocks+1]    */
    const int32_t *f_row, *f_start, *f_n;  /* [n_rows]        */
} sslrec_swept_t;              /* host memory; arrays on the device */

/* pack_override / val_override [n_elem] and w_steps_override [16*n_blocks] (all nullable) multiply an edge-dropped
 * or re-valued view. */
/* d = the tables' embedding size: A->d, or 2 / 4 / 8 times A->d -- then the product runs as d / A->d launches, one per
 * block of A->d embedding columns of the [N, d] tables (a table wider than the LDS holds: sslrec_plan_layout falls back
 * to such a layout before it falls back to the streamed kernel). */
int sslrec_swept_deferred_sum_ok(const sslrec_swept_t *A);      /* 1: launches on A take sslrec_epilogue_t.sum_in (see there) */
int sslrec_spmm_swept_f32(const sslrec_swept_t *A, const int32_t *pack_override, const float *val_override,
                          const int32_t *w_steps_override, const float *X, int32_t d, float *Y,
                          const sslrec_epilogue_t *epi, void *stream);

/* sslrec_spmm_swept_f32 with one of two by-products of a training step compiled into the flush (the LightGCN step, lightgcn.py:38-56:
 * forward products, reg_weight * |E0|^2, backward products with the regularizer's gradient).  Same arguments, and the same bits in
 * Y / acc_out as sslrec_spmm_swept_f32 with the same epilogue; `step->flags` is exactly one of
 *   SSLREC_STEP_SUMSQ       the launch ALSO writes sumsq_out[0] = sumsq_weight * sum of the squares of the n_rows * d elements of
 *                           epi->acc_in.  Every output row is flushed exactly once and its acc_in row is in registers there, so the
 *                           sum costs 4 FMAs per lane and row and the launch and table read of sslrec_sumsq_fwd_f32 go away.
 *                           Deterministic: lanes, waves, workgroups and the launch are each added in a fixed order (the workgroup that
 *                           finishes last adds the workgroups' partials: the scheme of sslrec_sumsq_fwd_f32), so two launches on one
 *                           layout give the same bits; the order is not sslrec_sumsq_fwd_f32's, so the two may differ by rounding.
 *                           Needs a plain valued launch: none of epi->axpy_x, x_row_bits, SSLREC_SCALE_PATTERN.
 *                           sumsq_ws: sslrec_sumsq_ws_bytes() bytes, zero at entry (once: every launch leaves its ticket counters
 *                           zero again); it may be the workspace of sslrec_sumsq_fwd_f32 as long as the launches are ordered.
 *   SSLREC_STEP_AXPY_BATCH  needs epi->axpy_x.  The axpy_x rows are requested beside the acc_in rows, four flush passes at a time,
 *                           instead of one dependent load per output row; valued and pattern launches.  The sumsq_* fields are unused.
 * Both need: sslrec_swept_step_ok(A) == 1 (the one-workgroup-per-CU build, A->d in 32 .. 256), d == A->d (no embedding-column passes),
 * epi->acc_in / acc_out and epi->n_sum_in == 0 -- otherwise SSLREC_E_BADARG and nothing is launched: the caller asks the predicate
 * first and keeps sslrec_spmm_swept_f32 (and sslrec_sumsq_fwd_f32) everywhere else. */
#define SSLREC_STEP_SUMSQ 1
#define SSLREC_STEP_AXPY_BATCH 2
typedef struct {
    float *sumsq_ws;
    float *sumsq_out;
    float sumsq_weight;
    int32_t flags;
} sslrec_swept_step_t;
int sslrec_swept_step_ok(const sslrec_swept_t *A);              /* 1: launches on A can take sslrec_spmm_swept_step_f32 */
int sslrec_spmm_swept_step_f32(const sslrec_swept_t *A, const int32_t *pack_override, const float *val_override,
                               const int32_t *w_steps_override, const float *X, int32_t d, float *Y,
                               const sslrec_epilogue_t *epi, const sslrec_swept_step_t *step, void *stream);

/* One product, several epilogues: SimGCL's three views (simgcl.py:29-31: two perturbed forwards + a clean one)
 * start from the SAME A.E0, so their first layer is one launch whose flush applies up to SSLREC_MAX_VIEWS
 * (noise, acc_in, acc_out, Y) sets; noise[k] NULL = clean view.  (The mirror image holds for the gradient of that
 * layer: A^T applied once to the sum of the views' gradients.) */
#define SSLREC_MAX_VIEWS 4
typedef struct sslrec_epilogue_views {
    int32_t n_views; float eps;
    float *Y[SSLREC_MAX_VIEWS];
    const float *noise[SSLREC_MAX_VIEWS];
    const float *acc_in[SSLREC_MAX_VIEWS];
    float *acc_out[SSLREC_MAX_VIEWS];
    const uint64_t *philox;                      /* device-side noise for the views with philox_noise[k] != 0 */
    uint32_t philox_stream[SSLREC_MAX_VIEWS];
    int32_t philox_noise[SSLREC_MAX_VIEWS];
    const float *row_scale; int32_t scale_flags;   /* SSLREC_SCALE_Y / SSLREC_SCALE_ACC for every view (see sslrec_epilogue_t; ABI 6) */
} sslrec_epilogue_views_t;     /* host memory */
int sslrec_spmm_swept_views_f32(const sslrec_swept_t *A, const float *X, int32_t d,
                                const sslrec_epilogue_views_t *views, void *stream);

/* EdgeDrop on the swept layout (replaces EdgeDrop.forward, models/aug_utils.py:18-31): keep[] is the
 * reference's per-entry mask in the ORIGINAL COO order, edge_map[e] the COO entry that governs element e
 * (unused for pads).  Every lane group's stream is compacted inside its own slots: kept entries (values times
 * scale) move to the front in their original order, the rest becomes pads; w_steps_out receives the new step
 * counts (longest compacted stream of each wave, rounded up to 4). */
int sslrec_swept_compact(const sslrec_swept_t *A, const int32_t *edge_map, const uint8_t *keep, float scale,
                         int32_t *pack_out, float *val_out, int32_t *w_steps_out, void *stream);

/* Device-side augmentation RNG (perf mode; the reference draws on the CPU generator, models/aug_utils.py:28,130, and
 * the parity mode of this library consumes exactly those draws).  philox_state = 2 x uint64 in DEVICE memory:
 * {seed, step}.  A uniform is a pure function of (seed, step, stream, element): `stream` is a per-call constant chosen
 * by the host (distinct per augmentation call of a training step), element = the COO entry id (EdgeDrop: forward and
 * transposed views of one call therefore agree) or the row-major float index / 4 of the output table (EmbedPerturb);
 * u = (x >> 8) * 2^-24.  sslrec_philox_advance does step += 1 on the device -- call it once per training step; it is a
 * kernel, so a captured hipGraph draws fresh numbers on every replay. */
int sslrec_philox_advance(uint64_t *philox_state, void *stream);
/* the noise of call `philox_stream` written out: out[4i .. 4i+3] = the four uniforms of float group i (n a multiple of 4).
 * What the epilogues compute on the fly; for tests and for callers that want the dense EmbedPerturb tensor. */
int sslrec_philox_fill_f32(const uint64_t *philox_state, uint32_t philox_stream, float *out, size_t n, void *stream);
/* out[r] = sum over the d draws of row r of that noise squared (d a multiple of 4): the full-row norm of EmbedPerturb for a
 * launch that only holds a column slice of the row */
int sslrec_philox_row_sumsq(const uint64_t *philox_state, uint32_t philox_stream, int32_t n_rows, int32_t d, float *out, void *stream);
/* out[r] (+)= sum_c x[r, c]^2 for a row-major [n_rows, d] table (d a multiple of 4): a rank's share of the same norm for SUPPLIED noise */
int sslrec_row_sumsq_f32(const float *x, int32_t n_rows, int32_t d, float *out, void *stream);
/* The reference's own draws on the device (parity mode): the CPU generator behind `t.rand` (models/aug_utils.py:28,130) is
 * MT19937; mt_state = uint32[625] in DEVICE memory = its 624 state words + the index of the next output in the current
 * block (624 = block exhausted), as found in torch.get_rng_state().  The calls write the next n numbers of that stream --
 * (y & 0xFFFFFF) * 2^-24 per tempered output, bit-identical to `t.rand(n)` on the host -- and leave mt_state advanced by
 * n.  One workgroup (the stream is sequential); capturable in a hipGraph. */
int sslrec_mt19937_uniform_f32(uint32_t *mt_state, float *out, int64_t n, void *stream);
/* the same stream turned into EdgeDrop's mask: keep_out[i] = floor(u_i + keep_rate) != 0 */
int sslrec_mt19937_keep_mask(uint32_t *mt_state, float keep_rate, uint8_t *keep_out, int64_t n, void *stream);
/* The same stream from many workgroups.  One step of MT19937 is a linear map F of the state bits over GF(2); with
 * g = x^J mod phi (phi = the generator's characteristic polynomial, degree 19937) the state J words ahead is g(F) state =
 * the XOR of the 624-word windows at the set bits of g over the NEXT 19937 + 623 words.  The host computes the g's
 * (sslrec_amd/mt_jump.py; a polynomial = uint32[624], bit i = coefficient of x^i); the *_par calls take a two-level
 * table -- polys[(fan1-1) + (fan2-1)][624]: x^(624 B j) for j = 1..fan1-1, then x^(624 B fan1 k) for k = 1..fan2-1 --
 * derive the states at blocks B, 2B, ... (two launches) and give every stretch of B blocks its own workgroup: the same
 * numbers as the one-workgroup calls, the same state afterwards, any n (passes of fan1*fan2 stretches).
 * ws: sslrec_mt19937_par_ws_bytes(fan1, fan2) bytes. */
int sslrec_mt19937_jump_poly(const uint32_t *poly, const uint32_t *state_in, uint32_t *state_out, void *stream);
size_t sslrec_mt19937_par_ws_bytes(int32_t fan1, int32_t fan2);
int sslrec_mt19937_uniform_par_f32(uint32_t *mt_state, const uint32_t *polys, int32_t fan1, int32_t fan2, int64_t stretch_blocks,
                                   uint32_t *ws, float *out, int64_t n, void *stream);
int sslrec_mt19937_keep_mask_par(uint32_t *mt_state, const uint32_t *polys, int32_t fan1, int32_t fan2, int64_t stretch_blocks,
                                 uint32_t *ws, float keep_rate, uint8_t *keep_out, int64_t n, void *stream);
/* EdgeDrop with the mask computed in place: entry k is kept iff floor(u_k + keep_rate) != 0 (aug_utils.py:28-29) */
int sslrec_swept_compact_philox(const sslrec_swept_t *A, const int32_t *edge_map, float keep_rate,
                                const uint64_t *philox_state, uint32_t philox_stream, float scale,
                                int32_t *pack_out, float *val_out, int32_t *w_steps_out, void *stream);
/* EdgeDrop on the row-bundled layout: val_out[e] = keep(edge_map[e]) ? A->val[e] * scale : 0 -- the mask given (keep != NULL, one byte per
 * entry) or computed (keep == NULL: Philox, as above).  Hand val_out to sslrec_spmm_bundled_f32 as `val_override`: a zero-valued element
 * contributes exactly nothing (no compaction: the view runs the full stream length).  edge_map: sslrec_plan_edge_map(plan, d, STREAMED). */
int sslrec_bundled_drop_values(const sslrec_bundled_t *A, const int32_t *edge_map, const uint8_t *keep, float keep_rate,
                               const uint64_t *philox_state, uint32_t philox_stream, float scale, float *val_out, void *stream);
/* The same views COMPACTED (round 5; replaces EdgeDrop.forward, models/aug_utils.py:18-31, on the row-bundled layout): every row of a
 * bundle keeps its kept entries in their order, a bundle runs for the longest of its compacted rows and the bundles of a stream move up
 * behind each other, so a keep-0.5 view gathers about half of what the zero-valued form gathers.  col_out / val_out [A->n_elem],
 * b_steps_out [A->n_bundles], w_blocks_out [A->n_waves] (64-element blocks of every stream still in use) go to
 * sslrec_spmm_bundled_view_f32 as the four overrides.  Sums equal the zero-valued form's bit for bit (same entries, same order). */
int sslrec_bundled_compact(const sslrec_bundled_t *A, const int32_t *edge_map, const uint8_t *keep, float scale, int32_t *col_out,
                           float *val_out, int32_t *b_steps_out, int32_t *w_blocks_out, void *stream);
int sslrec_bundled_compact_philox(const sslrec_bundled_t *A, const int32_t *edge_map, float keep_rate, const uint64_t *philox_state,
                                  uint32_t philox_stream, float scale, int32_t *col_out, float *val_out, int32_t *b_steps_out,
                                  int32_t *w_blocks_out, void *stream);
int sslrec_edge_drop_compact_philox(const sslrec_csr_t *A, const int32_t *edge_map, float keep_rate,
                                    const uint64_t *philox_state, uint32_t philox_stream, float scale,
                                    int32_t *col_out, float *val_out, int32_t *r_len_out, int32_t *w_len_out, void *stream);

/* Edge dropout without rebuilding the matrix (replaces EdgeDrop.forward,
 * models/aug_utils.py:18-31: boolean-index values/indices, rebuild COO).
 * keep[k] (uint8, 0/1) is the reference's per-entry mask in the ORIGINAL COO entry order;
 * edge_map[e] gives, for element e of col[], the COO entry whose mask bit governs it (the
 * entry itself for the forward matrix, the transposed entry for the backward matrix; unused
 * for pads).  Kept entries of every row segment are re-packed into consecutive slots of the
 * same stream (same w_start, same element mapping) in col_out / val_out [n_elem];
 * r_len_out / w_len_out receive the new lengths in loads (a fully dropped row keeps a
 * zero-length segment and is written as zeros);
 * scale multiplies kept values (1/keep_rate when EdgeDrop(resize_val=True), else 1). */
int sslrec_edge_drop_compact(const sslrec_csr_t *A, const int32_t *edge_map,
                             const uint8_t *keep, float scale,
                             int32_t *col_out, float *val_out, int32_t *r_len_out,
                             int32_t *w_len_out, void *stream);

/* ------------------------------------------------------------------------------------
 * Native plan builder (host C++ inside the library; sslrec_amd/csrc/plan.cpp).  The reference converts its
 * uncoalesced COO adjacency (data_utils/data_handler_general_cf.py:70-73) to CSR inside EVERY torch.spmm call
 * (models/general_cf/lightgcn.py:28-29); here a caller hands over the matrix once -- as COO entries in any order or
 * as plain (rowptr, col, val) -- and receives the sslrec_swept_t / sslrec_csr_t layouts above.
 *   build_coo : entries sorted by (row, column), stable (duplicates kept in input order = the summation order)
 *   build_csr : entries of a row keep the order they are given in
 *   layout    : builds, on the host, the layout for embedding size d.  kind AUTO picks the column-swept layout when
 *               the output table fits the chip's LDS and the streamed one otherwise; returns the kind built (> 0)
 *               or a negative error.  flags: SSLREC_PLAN_NO_XCD_SPLIT keeps the two row classes of a bipartite
 *               adjacency on all XCDs.
 *   host_array: named host arrays of a layout ("pack","val","w_start","w_steps","wf_ptr","cf_ptr","f_row","f_start","f_n",
 *               "edge_map","elem_host","csr_pos_host" (f_ptr of ABI 2 became "wf_ptr" + "cf_ptr") / "col","val","w_start","w_len","r_ptr","r_len","r_dst","long_row",
 *               "long_ptr","edge_map",...; d = 0: "rowptr","col","val","perm" of the CSR) for callers that manage
 *               device memory themselves (the Python host does, through PyTorch's allocator)
 *   upload    : hipMalloc + copy of a layout; afterwards swept()/csr()/edge_map() return device-side descriptors and
 *               sslrec_plan_spmm_f32 multiplies with whichever kernel the layout belongs to.
 * edge_map[e] = index of the INPUT entry behind element e (-1 for pads): feed it to sslrec_swept_compact /
 * sslrec_edge_drop_compact with a per-input-entry keep mask. */
typedef struct sslrec_plan sslrec_plan_t;      /* opaque, host memory */
#define SSLREC_PLAN_AUTO 0
#define SSLREC_PLAN_SWEPT 1
#define SSLREC_PLAN_STREAMED 2
#define SSLREC_PLAN_BUNDLED 3      /* what kind STREAMED builds at d = 8 / 16 (and at 32 on request): reported by sslrec_plan_info */
#define SSLREC_PLAN_NO_XCD_SPLIT 1
typedef struct sslrec_plan_info {
    int32_t n_rows, n_cols; int64_t nnz;
    int32_t kind, d, xcd_split;
    int32_t n_elem, n_blocks, n_slots, n_streams, n_rseg, n_long;
    int64_t xcd_col_pairs;      /* swept layout with the XCD split: sum over the 8 XCDs of the DISTINCT columns their output rows reference
                                   (x 4 d bytes = what the XCDs' L2s pull through the fabric per launch when every line is fetched once per XCD) */
} sslrec_plan_info_t;
int sslrec_plan_build_coo(const int64_t *rows, const int64_t *cols, const float *vals, int64_t nnz, int32_t n_rows,
                          int32_t n_cols, sslrec_plan_t **out);                                  /* host pointers */
int sslrec_plan_build_csr(const int64_t *rowptr, const int32_t *col, const float *val, int32_t n_rows, int32_t n_cols,
                          sslrec_plan_t **out);                                                  /* host pointers */
int sslrec_plan_set_option(sslrec_plan_t *p, const char *name, int64_t value);   /* "seg_max": chunk cap of long rows in the
                                                        streamed layout; "n_streams": its number of work streams (0 = automatic);
                                                        "swept_blocks" 0 / 256 / 512; "xcd_balance" per mille; "swept_passes" 0 / 1:
                                                        allow a swept layout of d/2, d/4 ... columns run in embedding-column passes;
                                                        "xcd_cluster": row -> XCD co-clustering of the swept layout (rows that share
                                                        columns on the same XCD; same results bit for bit, only the fabric traffic
                                                        changes): 0 = never, 1..16 = always, that many refinement passes, 17 = automatic
                                                        (the default): kept when it lowers the distinct (XCD, column) pairs by > 25 % */
int sslrec_plan_layout(sslrec_plan_t *p, int32_t d, int32_t kind, int32_t flags);
/* the calls below address the layout of (d, kind); kind AUTO = the swept layout when one was built, else the streamed */
int sslrec_plan_info(const sslrec_plan_t *p, int32_t d, int32_t kind, sslrec_plan_info_t *info);
int sslrec_plan_host_array(const sslrec_plan_t *p, int32_t d, int32_t kind, const char *name, const void **ptr, int64_t *count,
                           int32_t *elem_bytes);
int sslrec_plan_upload(sslrec_plan_t *p, int32_t d, int32_t kind, void *stream);
const sslrec_swept_t *sslrec_plan_swept(const sslrec_plan_t *p, int32_t d);
const sslrec_csr_t *sslrec_plan_csr(const sslrec_plan_t *p, int32_t d);
const sslrec_bundled_t *sslrec_plan_bundled(const sslrec_plan_t *p, int32_t d);
const int32_t *sslrec_plan_edge_map(const sslrec_plan_t *p, int32_t d, int32_t kind);
int sslrec_plan_spmm_f32(const sslrec_plan_t *p, int32_t d, const float *X, float *Y, const sslrec_epilogue_t *epi,
                         void *stream);
void sslrec_plan_free(sslrec_plan_t *p);

/* Diagnostic, not an operator (no reference counterpart): while enabled, every launch of the column-swept kernel records per
 * wave the 100 MHz wall clock at the start of each metadata block (slots 0..28), at the end of its sweep (29) and at the
 * start (30) and end (31) of its flush, for the last 4 launches.  enable != 0 with host_out == NULL starts recording for
 * layouts of n_waves = 16 * n_blocks waves; a call with host_out copies the ring [4][n_waves][32] out; enable == 0 stops and
 * frees.  Returns the number of launches recorded so far (tools/spmm_trace.py; EXPERIMENTS.md B 4.1b's time line). */
int sslrec_debug_swept_trace(int enable, unsigned long long *host_out, int n_waves);

/* Measurement hook, not an operator: in-kernel launch timing that survives hipGraph capture (HIP events cannot be recorded
 * inside a captured graph's kernels, and a replayed step is what bench.py --gpus N times).  `record` = 4 x uint64 in DEVICE
 * memory, initialised to {~0, 0, 0, 0}; the NEXT SpMM launch of this thread (either kernel; all column passes of one call)
 * is handed the record: every workgroup stamps the 100 MHz wall clock when it starts (minimum kept in record[0]) and when
 * it has finished (its stores drained); the last one to finish adds (its clock - the minimum) to record[1] and 1 to record[3],
 * and resets record[0].  So after K replays record[1] / record[3] is the kernel's average duration in 10 ns ticks, first
 * workgroup start to last workgroup end -- the quantity rocprofv3's kernel trace reports.  NULL cancels a pending record. */
int sslrec_debug_stamp_next_launch(unsigned long long *record);
/* rate of that wall clock on the current device in kHz (hipDeviceAttributeWallClockRate; 100000 on MI355X), <= 0 on error */
int sslrec_debug_wall_clock_khz(void);

/* ------------------------------------------------------------------------------------
 * BPR loss over gathered rows (replaces the three gathers + cal_bpr_loss,
 * models/general_cf/lightgcn.py:49-52 and models/loss_utils.py:7-10; variant 1 is
 * LightGCL's -log(sigmoid(pos-neg)), models/general_cf/lightgcl.py:106-108).
 * Ta/Tp/Tn are row-major [*, d] tables; ia/ip/in are int64 row ids or NULL (= row b).
 *   fwd: loss_out[0] = sum_b f(<a_b,n_b> - <a_b,p_b>) / divisor  (divisor = the batch size folds the caller's `/ B`,
 *        lightgcn.py:52; 1 for the plain sum);   ws: sslrec_bpr_ws_bytes(B) bytes that MUST BE ZERO at entry -- it starts with ticket
 *        counters: the workgroup that finishes last adds the partial sums (fixed order) inside the same launch; the call leaves the
 *        counters zero again, so a workspace zeroed once can be reused call after call (not by two streams at the same time)
 *   fwd_total: the same launch also writes loss_out2[1] = loss_out2[0] + add_in[0] (add_in: a device scalar, e.g. the
 *        regularizer term: `bpr_loss + reg_loss` of lightgcn.py:54 without an elementwise launch of its own)
 *   bwd: dTa[ia[b]] += g*..., etc.  With an index array the contributions are added DETERMINISTICALLY (per destination
 *        row in ascending sample order: bit-reproducible, duplicates allowed, tables may alias) using
 *        ws = sslrec_bpr_bwd_ws_bytes(B, d) bytes; ws == NULL or 3B > 16384 falls back to atomic adds.  Without an
 *        index array: a plain store to row b.  gscale = upstream gradient (already divided by B when the caller averages). */
size_t sslrec_bpr_ws_bytes(int32_t B);
size_t sslrec_bpr_bwd_ws_bytes(int32_t B, int32_t d);
int sslrec_bpr_fwd_f32(const float *Ta, const int64_t *ia, const float *Tp, const int64_t *ip,
                       const float *Tn, const int64_t *in, int32_t B, int32_t d, int32_t variant,
                       float divisor, float *ws, float *loss_out, void *stream);
int sslrec_bpr_fwd_total_f32(const float *Ta, const int64_t *ia, const float *Tp, const int64_t *ip,
                             const float *Tn, const int64_t *in, int32_t B, int32_t d, int32_t variant,
                             float divisor, const float *add_in, float *ws, float *loss_out2, void *stream);
int sslrec_bpr_bwd_f32(const float *Ta, const int64_t *ia, const float *Tp, const int64_t *ip,
                       const float *Tn, const int64_t *in, int32_t B, int32_t d, int32_t variant, float divisor,
                       const float *gscale_dev, float *dTa, float *dTp, float *dTn, void *ws, void *stream);
/* The same backward on a workspace that is KEPT between calls (same B and d, one stream at a time): sslrec_bpr_bwd_table_init clears
 * the scatter table inside ws once; sslrec_bpr_bwd_kept_f32 then needs no clearing launch -- the reduction hands every slot it used
 * back cleared -- two launches per call instead of three.  3B <= 16384, d <= 256, ws != NULL.
 * zero_table / zero_elems (nullable / 0; all three roles indexed, 16-byte aligned, a multiple of 4 floats): the gradient table(s) the
 * rows are added into -- one contiguous range covering dTa, dTp, dTn -- zeroed by the staging launch itself instead of by a fill
 * launch of the caller's (37 MB at amazon-book size: it runs under the staging's latency). */
int sslrec_bpr_bwd_table_init(void *ws, int32_t B, int32_t d, void *stream);
int sslrec_bpr_bwd_kept_f32(const float *Ta, const int64_t *ia, const float *Tp, const int64_t *ip,
                            const float *Tn, const int64_t *in, int32_t B, int32_t d, int32_t variant, float divisor,
                            const float *gscale_dev, float *dTa, float *dTp, float *dTn, void *ws, float *zero_table,
                            size_t zero_elems, void *stream);
/* The backward STAGED BY THE FORWARD launch (a forward whose backward is known to follow): two launches per step instead of three.
 *   fwd_staged : everything the forward does (loss_out[0], and loss_out[1] = loss_out[0] + add_in[0] when add_in != NULL; same
 *        ws and the same bits), and for every triple the three gradient rows for an upstream gradient of exactly 1, staged in the KEPT
 *        workspace bwd_ws (sslrec_bpr_bwd_ws_bytes, cleared by sslrec_bpr_bwd_table_init or left clean by the previous call) with
 *        their destination rows of dTa / dTp / dTn registered; zero_table / zero_elems as in bwd_kept.  All three roles indexed,
 *        3B <= 16384, d <= 256.  The rows are loaded once for the loss and the gradient.
 *   bwd_from_staged : adds the staged rows, each multiplied by gscale_dev[0], into the registered destinations (deterministic, as
 *        bwd) and leaves bwd_ws's table clean.  For gscale = 1 the result has the bits of bwd_kept.  Until this call (or a
 *        sslrec_bpr_bwd_table_init) bwd_ws's table holds the staged keys: no other call may use it in between. */
int sslrec_bpr_fwd_staged_f32(const float *Ta, const int64_t *ia, const float *Tp, const int64_t *ip,
                              const float *Tn, const int64_t *in, int32_t B, int32_t d, int32_t variant, float divisor,
                              const float *add_in, float *ws, float *loss_out, float *dTa, float *dTp, float *dTn,
                              void *bwd_ws, float *zero_table, size_t zero_elems, void *stream);
int sslrec_bpr_bwd_from_staged_f32(int32_t B, int32_t d, const float *gscale_dev, void *bwd_ws, void *stream);

/* ------------------------------------------------------------------------------------
 * InfoNCE against ALL rows of a view (replaces cal_infonce_loss,
 * models/loss_utils.py:30-39, called at simgcl.py:49 / sgl.py:57-59; variant 1 is
 * LightGCL's un-normalized form, models/general_cf/lightgcl.py:114-118).
 *
 *   variant 0:  x^ = x / sqrt(1e-8 + |x|^2) for e1, e2, all
 *               loss = sum_b [ -<e1^_b,e2^_b>/temp + log sum_j exp(<e1^_b, all^_j>/temp) ]
 *   variant 1:  no normalization;
 *               loss = sum_b [ -clamp(<e1_b,e2_b>/temp,-5,5) + log(sum_j exp(<e1_b,all_j>/temp) + 1e-8) ]
 *               (the caller divides by B for the reference's .mean()).
 * e1 = T1[i1[b]], e2 = T2[i2[b]] (index arrays nullable = row b); all = ALL[0..M).
 * The B x M score matrix is never materialized: FP32 MFMA tiles, exp and row sums stay
 * in registers.  d must be 32, 64 or 128.
 *   fwd: loss_out[0] = loss;  ws (sslrec_infonce_ws_bytes) keeps the normalized operands and
 *        the B row sums; the SAME ws must be handed to bwd.
 *   bwd: dE1,dE2 are dense [B,d] (caller scatters), dALL is dense [M,d]; all three are
 *        overwritten.  gscale_dev: upstream gradient scalar on device.
 * `variant` carries three fields, and the forward and backward calls of one evaluation must pass the SAME value:
 *   bits 0..7    0 / 1 as above;
 *   bits 8..15   arithmetic of the B x M products (SSLREC_INFONCE_PREC_*; 0 = the process default: the environment variable
 *                SSLREC_INFONCE_PRECISION, else h3 for variant 0 and x6 for variant 1; h3 -- by default or by name -- runs as x6 when
 *                temp < log2(e) / 15.5 = 0.0931, where its exponent bias would go negative).  x6 = operands as three bf16 planes, six bf16-MFMA terms per product with fp32
 *                accumulation (fp32-level error, held to the fp32 tolerances by every parity test); fp32 = v_mfma_f32_32x32x2_f32;
 *                the other modes drop terms and are opt-in;
 *   bit 16       SSLREC_INFONCE_FWD_W: the forward call also accumulates the anchor-gradient sums W_b = sum_j exp(s_bj) all_j
 *                (they depend neither on the upstream gradient nor on the row sums) in the workspace, from the SAME score tiles
 *                its row sums come from, and the backward call does not recompute them: the B x M score products are formed
 *                twice per forward + backward instead of three times.  Set it when a backward call will follow (a caller that
 *                only wants the loss leaves it clear: the forward then costs half as much). */
#define SSLREC_INFONCE_PREC_DEFAULT 0
#define SSLREC_INFONCE_PREC_X6 1
#define SSLREC_INFONCE_PREC_FP32 2
#define SSLREC_INFONCE_PREC_X36 3
#define SSLREC_INFONCE_PREC_X3 4
#define SSLREC_INFONCE_PREC_X63 5
#define SSLREC_INFONCE_PREC_X6A 6
#define SSLREC_INFONCE_PREC_H3 7        /* two fp16 planes / three fp16-MFMA terms per product (22-bit operands; variant 0 only, variant 1 runs x6) */
#define SSLREC_INFONCE_FWD_W (1 << 16)
size_t sslrec_infonce_ws_bytes(int32_t B, int32_t M, int32_t d);
int sslrec_infonce_fwd_f32(const float *T1, const int64_t *i1, const float *T2, const int64_t *i2,
                           int32_t B, const float *ALL, int32_t M, int32_t d, float temp,
                           int32_t variant, float *ws, float *loss_out, void *stream);
int sslrec_infonce_bwd_f32(const float *T1, const int64_t *i1, const float *T2, const int64_t *i2,
                           int32_t B, const float *ALL, int32_t M, int32_t d, float temp,
                           int32_t variant, float *ws, const float *gscale_dev,
                           float *dE1, float *dE2, float *dALL, void *stream);

/* Backward with the scatter of the gathered rows' gradients inside (the index_put backward of `T1[i1]` / `T2[i2]`, simgcl.py:32-37):
 * dE [2B, d] receives dE1 then dE2; for a role with an index array the rows are ADDED into dT1 / dT2 (the caller's gradient
 * tables: zero-initialised, or -- T2 being `all` itself, the call shape of simgcl.py:49 / sgl.py:57-59 -- dT2 = dALL), duplicates
 * in ascending sample order (bit-reproducible).  The rows are registered by the launch that writes dE, one reduction launch adds
 * both roles; the table
 * (scatter_ws: sslrec_scatter_ws_bytes(2B) bytes) is cleared by the backward's first kernel.  2B <= 16384. */
int sslrec_infonce_bwd_scatter_f32(const float *T1, const int64_t *i1, const float *T2, const int64_t *i2,
                                   int32_t B, const float *ALL, int32_t M, int32_t d, float temp,
                                   int32_t variant, float *ws, const float *gscale_dev, float *dE,
                                   float *dT1, float *dT2, float *dALL, void *scatter_ws, void *stream);

/* The same InfoNCE with `all` ROW-SHARDED over ranks (the reference has no multi-GPU
 * path -- this is the sharded form of loss_utils.py:30-39).  Every rank passes the same B anchor/positive
 * rows and ITS M rows of `all`; Z_b = sum_j exp(.) and W_b = sum_j exp(.) a_j are sums over j, so:
 * (`variant` as above, the same value in all four calls; with SSLREC_INFONCE_FWD_W step 1 also leaves this rank's W partials in ws
 * and step 3 only forms dALL and sums them.)
 *   1. shard_rowsum:      z_part[B]   = partial row sums over the local rows      -> host all-reduces z
 *   2. shard_loss:        loss_out[0] = sum_b(-pos_b + log z_total[b])  (same value on every rank)
 *   3. shard_bwd:         dALL[M,d] (complete for the local rows), w_part[B,d]     -> host all-reduces w
 *   4. shard_finish_bwd:  dE1,dE2 [B,d] from w_total (same values on every rank)
 * ws: sslrec_infonce_ws_bytes(B, M, d) with the LOCAL M, carried through the four calls. */
int sslrec_infonce_shard_rowsum_f32(const float *T1, const int64_t *i1, const float *T2, const int64_t *i2,
                                    int32_t B, const float *ALL, int32_t M, int32_t d, float temp,
                                    int32_t variant, float *ws, float *z_part, void *stream);
int sslrec_infonce_shard_loss_f32(int32_t B, int32_t M, int32_t d, int32_t variant, float *ws,
                                  const float *z_total, float *loss_out, void *stream);
int sslrec_infonce_shard_bwd_f32(int32_t B, int32_t M, int32_t d, float temp, int32_t variant, float *ws,
                                 const float *gscale_dev, float *w_part, float *dALL, void *stream);
int sslrec_infonce_shard_finish_bwd_f32(int32_t B, int32_t M, int32_t d, float temp, int32_t variant,
                                        float *ws, const float *gscale_dev, const float *w_total,
                                        float *dE1, float *dE2, void *stream);

/* Sum of squares of a parameter table and its gradient (replaces `W.norm(2).square()` per parameter in
 * reg_params, models/loss_utils.py:20-24): out[0] = weight * sum_i x_i^2 ;  dx = 2 * gscale * weight * x  (weight folds
 * the caller's `reg_weight *`, lightgcn.py:53; 1 for the plain sum).
 * x and dx must be 16-byte aligned; ws: sslrec_sumsq_ws_bytes() bytes, zero at entry (once: the call leaves its ticket counters zero
 * again -- the one-launch reduction of sslrec_bpr_fwd_f32). */
size_t sslrec_sumsq_ws_bytes(void);
int sslrec_sumsq_fwd_f32(const float *x, size_t n, float weight, float *ws, float *out, void *stream);
int sslrec_sumsq_bwd_f32(const float *x, size_t n, float weight, const float *gscale_dev, float *dx, void *stream);

/* Step-level helpers of the one-node contrastive steps (ops.contrastive_step: SimGCL simgcl.py:39-55, SGL sgl.py:45-65 as ONE autograd
 * node with a hand-written backward): the scalar arithmetic and table additions PyTorch would run as stock elementwise launches.
 *   weighted_sum4 : out6[0] = ((w0 t0 + w1 t1) + w2 t2) + w3 t3, out6[1 + k] = w_k t_k, out6[5] = w1 t1 + w2 t2 (the loss and its logged
 *                   parts, simgcl.py:50-54: bpr, the two contrastive terms, the regularizer; t_k: device scalars, nullable = 0)
 *   scalar_scale2 : out2 = (a x, b x) of a device scalar x (the upstream gradient times the terms' weights)
 *   add_tables    : out = (a + b) [+ c] elementwise (c nullable; n a multiple of 4, 16-byte aligned; out may alias an input) */
int sslrec_weighted_sum4_f32(const float *t0, float w0, const float *t1, float w1, const float *t2, float w2, const float *t3, float w3,
                             float *out6, void *stream);
int sslrec_scalar_scale2_f32(const float *x, float a, float b, float *out2, void *stream);
int sslrec_add_tables_f32(const float *a, const float *b, const float *c, float *out, size_t n, void *stream);

/* Adam step over one parameter tensor (replaces torch.optim.Adam as the reference's Trainer uses it,
 * trainer/trainer.py:45-49,68).  state: 4 floats on the device, zero-initialised:
 * sslrec_adam_tick advances the step count t kept in state[0] and stores lr/(1-beta1^t), sqrt(1-beta2^t)
 * (computed in double); sslrec_adam_apply_f32 then does, per element and in one pass,
 *   g' = g + weight_decay*p;  m += (1-beta1)(g'-m);  v = beta2 v + (1-beta2) g'^2;
 *   p -= lr/(1-beta1^t) * m / (sqrt(v)/sqrt(1-beta2^t) + eps)
 * (hyper-parameters as doubles: 1-beta is rounded to fp32 once, from the double, like PyTorch does).
 * Call tick once per optimizer step, apply once per tensor (16-byte aligned). */
int sslrec_adam_tick(float *state, double lr, double beta1, double beta2, void *stream);
int sslrec_adam_apply_f32(float *p, const float *g, float *m, float *v, size_t n, const float *state,
                          double beta1, double beta2, double eps, double weight_decay, void *stream);

/* Rank-q products of LightGCL's SVD view (replaces `u_mul_s @ (vt @ E)` and its autograd backward,
 * models/general_cf/lightgcl.py:83-84; q <= 16).  M(k, n) = M[k*stride_q + n*stride_n] addresses a row-major [q,N]
 * factor (stride_q = N, stride_n = 1) or a row-major [N,q] factor (stride_q = 1, stride_n = q).
 *   reduce: out[q,d] = sum_n M(.,n) X[n,:]   (two-stage, fixed order: deterministic; ws: sslrec_rankq_ws_bytes)
 *   expand: Y[n,:]   = sum_k M(k,n) S[k,:] */
size_t sslrec_rankq_ws_bytes(int32_t q, int32_t d);
int sslrec_rankq_reduce_f32(const float *M, int64_t stride_q, int64_t stride_n, const float *X, int32_t N, int32_t d,
                            int32_t q, float *ws, float *out, void *stream);
int sslrec_rankq_expand_f32(const float *M, int64_t stride_q, int64_t stride_n, const float *S, int32_t N, int32_t d,
                            int32_t q, float *Y, void *stream);

/* ------------------------------------------------------------------------------------
 * All-rank evaluation: top-k unseen items per user (replaces full_predict + _mask_predict + t.topk,
 * models/general_cf/lightgcn.py:58-66, models/base_model.py:35-36, trainer/metrics.py:99-103).
 *   scores[u, i] = <UE[users[u]], IE[i]> in exact-fp32 MFMA tiles (d = 32, 64 or 128; from 2048 users on, on two fp16 planes per table with
 *   22-bit operands -- SSLREC_EVAL_PRECISION=fp32 / h3 forces either); items of the user's train row
 *   (trn_rowptr [n_user_rows + 1], trn_col sorted inside a row, int64, device; both NULL = nothing seen) are skipped --
 *   the reference gives them -1e8, i.e. they lose to every unseen item;  out_idx [n_users, k] int64, descending by
 *   score, ties by ascending item id, -1 where a user has fewer than k unseen items; out_val (nullable) the scores.
 *   users (nullable = rows 0..n_users-1): int64 row ids into UE.  k <= 64.  ws: sslrec_eval_topk_ws_bytes bytes.
 * Neither the [B, I] score matrix nor the dense train mask the reference copies from the host ever exists. */
/* full_predict + _mask_predict themselves (models/general_cf/lightgcn.py:58-66, models/base_model.py:35-36) -- the dense matrix is the
 * reference's plugin contract: out[u, i] = s (1 - m) - 1e8 m with s = <UE[users[u]], IE[i]> (exact-fp32 MFMA tiles, d = 32 / 64 / 128)
 * and m = train_mask[u, i] ([n_users, n_items] row-major, nullable = no mask; mask_elem_bytes 8 = int64 as the reference's .long()
 * batch, 4 = float32, 1 = uint8 / bool).  One pass: the mask is read once, the result written once, no intermediate matrix. */
int sslrec_full_predict_f32(const float *UE, const int64_t *users, int32_t n_users, const float *IE, int32_t n_items, int32_t d,
                            const void *train_mask, int32_t mask_elem_bytes, float *out, void *stream);
size_t sslrec_eval_topk_ws_bytes(int32_t n_users, int32_t n_items, int32_t k);
int sslrec_eval_topk_f32(const float *UE, const int64_t *users, int32_t n_users, const float *IE, int32_t n_items,
                         int32_t d, const int64_t *trn_rowptr, const int64_t *trn_col, int32_t k, void *ws,
                         int64_t *out_idx, float *out_val, void *stream);

/* Measurement aid (csrc/micro.hip; bench.py's `roofline.ceiling`): `blocks` workgroups of 16 waves gather random rows of the
 * [n_rows, row_bytes] table X (row_bytes 128 / 256 / 512; 8 loads in flight per wave, `iters` rounds); *n_gathers = rows fetched.
 * scratch: >= 16 KiB, never written. */
int sslrec_debug_gather_rows(const float *X, uint32_t n_rows, int32_t row_bytes, int32_t iters, int32_t blocks, float *scratch,
                             int64_t *n_gathers, void *stream);

/* Negative sampling (replaces PairwiseTrnData.sample_negs, data_utils/datasets_general_cf.py:13-20; SURVEY.md §8f
 * rank 3): negs_out[i] = an item drawn uniformly from [0, n_item) and redrawn while (users[i], item) is a train
 * interaction (trn_rowptr / trn_col as above).  Draws come from the Philox stream (philox_state, philox_stream) --
 * the reference's distribution, not its numpy random stream. */
int sslrec_sample_negs(const int64_t *users, int64_t n, const int64_t *trn_rowptr, const int64_t *trn_col, int32_t n_item,
                       const uint64_t *philox_state, uint32_t philox_stream, int64_t *negs_out, void *stream);

/* The SAME negative sampling on the host, continuing numpy's global MT19937 generator bit for bit (ABI 7): the
 * reference's loop `np.random.randint(item_num)` until `(u, iNeg) not in dokmat`, one interaction after the other
 * (data_utils/datasets_general_cf.py:13-20), consumes one 32-bit generator output per attempt (masked rejection).
 * HOST pointers throughout; no device work.  mt_key[624] / *mt_pos = `np.random.get_state()[1:3]`, advanced in place
 * (write them back with `np.random.set_state`); users int32 [n] (coomat.row); trn_rowptr int64 [n_user+1] / trn_col int32
 * ascending within a row = the train interactions (the dok matrix's keys); negs_out int32 [n]; n_draws (nullable) = generator
 * outputs consumed.  SSLREC_E_BADARG when a user has interacted with every item (the reference would not return). */
int sslrec_sample_negs_mt19937(uint32_t *mt_key, int32_t *mt_pos, const int32_t *users, int64_t n,
                               const int64_t *trn_rowptr, const int32_t *trn_col, int32_t n_user, int32_t n_item,
                               int32_t *negs_out, int64_t *n_draws);

/* rows of src [B,d] are added into dst[idx[b], :] (the index_put backward of the gathers at lightgcn.py:49-51 /
 * simgcl.py:32-37), duplicates in a fixed order (per destination in ascending b: bit-reproducible) with
 * ws = sslrec_scatter_ws_bytes(B) bytes; ws == NULL or B > 16384: atomic adds. */
size_t sslrec_scatter_ws_bytes(int32_t B);
int sslrec_scatter_add_rows_f32(const float *src, const int64_t *idx, int32_t B, int32_t d,
                                float *dst, void *ws, void *stream);

/* ------------------------------------------------------------------------------------
 * Learned edge weights (csrc/sddmm.hip): AdaptiveMask, models/aug_utils.py:73-79, as DCCF calls it behind four index_selects
 * that materialize [nnz, d] tensors, models/general_cf/dccf.py:83-90.  Here an ENTRY is one COO entry of the adjacency in the
 * caller's order (the numbering of EdgeDrop masks); every per-entry array is fp32 [nnz] in that order.  The pattern is a plan's
 * plain CSR on the device, int32: rowptr [n_rows + 1], col [nnz], perm [nnz] (CSR position -> entry id) and row_of_entry [nnz]
 * (CSR position -> row).  The transposed plan numbers the entries alike, so per-column sums are row sums over ITS CSR: no scatter,
 * no atomics, every sum in a fixed order.  Embedding sizes: 8, 16, 32, 64, 128, 256.
 * ---------------------------------------------------------------------------------- */

/* Sampled dense-dense product: out[perm[k]] = <A[row_of_entry[k], :], B[col[k], :]> * ra[row] * cb[col] for every CSR position k
 * (the gathers plus t.sum(head * tail, dim=1) of aug_utils.py:75 and dccf.py:83-84, one row gather per entry and side instead of
 * two [nnz, d] tensors).  A [n_rows, d], B [n_cols, d] row-major, may alias; ra [n_rows] / cb [n_cols] nullable (= 1): with the
 * inverse row norms the result is the cosine, without a normalized copy of the table (F.normalize, aug_utils.py:73-74).  Work is
 * split by entries, so a hub row does not serialize a wave. */
int sslrec_sddmm_f32(const int32_t *row_of_entry, const int32_t *col, const int32_t *perm, int32_t n_rows, int32_t n_cols, int32_t nnz,
                     const float *A, const float *B, int32_t d, const float *ra, const float *cb, float *out, void *stream);

/* Rows of more than SSLREC_EDGE_LONG_ROW entries get a workgroup of their own in the two row normalizations below: long_rows
 * [n_long] must then list exactly those rows (n_long = 0: every row is walked by one 16-lane group, whatever its length). */
#define SSLREC_EDGE_LONG_ROW 512

/* aug_utils.py:75-79: alpha = (c + 1) / 2, s_h = sum of alpha over row h, inv_s[h] = 1 / s_h (0 where that is not finite:
 * .pow(-1).nan_to_num(0, 0, 0)), w[e] = alpha[e] * inv_s[row(e)].  c, w [nnz] in entry order; inv_s [n_rows]. */
int sslrec_edge_rownorm_fwd_f32(const int32_t *rowptr, const int32_t *perm, int32_t n_rows, const int32_t *long_rows, int32_t n_long,
                                const float *c, float *w, float *inv_s, void *stream);

/* its backward (autograd of aug_utils.py:75-79): dc[e] = inv_s[h] / 2 * (dw[e] - sum over row h of w * dw), and the two per-node
 * sums the cosine's backward needs, p_head[h] = sum of dc * c over row h and p_tail[t] = sum of dc * c over the entries INTO t --
 * the latter over the transposed plan's CSR (rowptr_t [n_cols + 1], perm_t, long_rows_t).  dc [nnz]; p_head [n_rows]; p_tail [n_cols]. */
int sslrec_edge_rownorm_bwd_f32(const int32_t *rowptr, const int32_t *perm, int32_t n_rows, const int32_t *long_rows, int32_t n_long,
                                const int32_t *rowptr_t, const int32_t *perm_t, int32_t n_cols, const int32_t *long_rows_t,
                                int32_t n_long_t, const float *dw, const float *w, const float *inv_s, const float *c, float *dc,
                                float *p_head, float *p_tail, void *stream);

/* n[r] = 1 / max(||S[r, :]||_2, 1e-12), the factor of F.normalize (aug_utils.py:73-74); normalized (nullable) [n_rows, d] = n (.) S,
 * which the valued SpMMs of the backward multiply. */
int sslrec_row_invnorm_f32(const float *S, int32_t n_rows, int32_t d, float *n, float *normalized, void *stream);

/* Finish of the cosine's backward: with G[r, :] = sum over the entries of node r of dc * (normalized other end) -- one valued SpMM
 * per side -- dS[r, :] = n[r] * (G[r, :] - (p_a[r] + p_b[r]) * n[r] * S[r, :]); rows whose norm is below 1e-12 were divided by the
 * constant and get n[r] * G[r, :].  p_b nullable (two-table form: one side per table); dS may be G. */
int sslrec_cosine_finish_f32(const float *S, const float *n, const float *G, const float *p_a, const float *p_b, int32_t n_rows,
                             int32_t d, float *dS, void *stream);

/* ------------------------------------------------------------------------------------
 * Intent-aware aggregation of DCCF (csrc/intent.hip), models/general_cf/dccf.py:77-80:
 *     u_embeds, i_embeds = torch.split(all_embeds[i], [user_num, item_num], 0)
 *     u_int_embeds = torch.softmax(u_embeds @ user_intent, dim=1) @ user_intent.T
 *     i_int_embeds = torch.softmax(i_embeds @ item_intent, dim=1) @ item_intent.T
 *     int_layer_embeds = torch.concat([u_int_embeds, i_int_embeds], dim=0)
 * on the stacked table X [N, d] (fp32, row-major): rows [0, n_split) use C_u, rows [n_split, N) use C_i, both [d, K] row-major as the
 * parameters are stored.  d in {32, 64, 128}, 1 <= K <= 256, 0 <= n_split <= N; the matrix of an EMPTY range may be null.  Nothing
 * of size N x K is written to global memory: the prototype matrix stays in LDS, the products are exact-fp32 MFMAs, the softmax
 * subtracts the row maximum.  Every entry point returns SSLREC_E_BADARG before any launch for a null required pointer or a size
 * outside these ranges; N == 0 returns 0 without a launch. */

/* bytes of the backward's workspace (per-workgroup partial sums of dC); 0 for arguments out of range */
size_t sslrec_intent_ws_bytes(int32_t N, int32_t n_split, int32_t d, int32_t K);

/* Y [N, d] = softmax(X C) C^T; lse [N] (nullable) receives the log-sum-exp of every row's logits, which the backward needs */
int sslrec_intent_fwd_f32(const float *X, int32_t N, int32_t n_split, int32_t d, const float *C_u, const float *C_i, int32_t K, float *Y,
                          float *lse, void *stream);

/* From dY [N, d]: p = exp(X C - lse) recomputed, dp = dY C, dz = p (dp - <p, dp>), dX = dz C^T, dC = sum over the range's rows of
 * X_r^T dz + dY_r^T p.  dC_u / dC_i [d, K]: required for a non-empty range, zero-filled if given for an empty one.  No atomics:
 * per-workgroup sums in ws (sslrec_intent_ws_bytes), added in a fixed order by a second launch -- two runs give the same bits. */
int sslrec_intent_bwd_f32(const float *X, const float *dY, const float *lse, int32_t N, int32_t n_split, int32_t d, const float *C_u,
                          const float *C_i, int32_t K, float *dX, float *dC_u, float *dC_i, void *ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * Hypergraph layer of HCCF (csrc/hyper.hip), models/general_cf/hccf.py:43-44, 48-49 and HGNNLayer.forward :105-107:
 *     uu_hyper = self.user_embeds @ self.user_hyper_embeds * self.mult
 *     hyper_user_embeds = self.hgnn_layer(F.dropout(uu_hyper, p=1-keep_rate), embeds_list[-1][:self.user_num])
 *         hids = self.act(adj.T @ embeds);  embeds = self.act(adj @ hids)              (act = LeakyReLU(leaky))
 * and the same for the items, on the stacked tables E (the parameters) and X (the layer's input), both [N, d] fp32 row-major: rows
 * [0, n_split) use W_u, rows [n_split, N) use W_i, both [d, K] row-major as the parameters are stored.  d in {32, 64, 128},
 * 1 <= K <= 256 except d = 128 with K > 128 (two [d, K] matrices exceed LDS: SSLREC_E_BADARG, workspace size 0), 0 <= n_split <= N,
 * leaky > 0, 0 < keep_rate <= 1; the pointers of an EMPTY range may be null.  Nothing of size N x K is written: A = dropout(E W mult) is
 * recomputed wherever it is needed, and its mask is computed from the Philox state (see "device-side augmentation RNG"):
 *     keep(row, k) = floor(u + keep_rate) != 0,  u = uniform number row * 4 ceil(K / 4) + k of call philox_stream
 * (sslrec_philox_fill_f32 writes the same numbers out); a kept element is scaled by mult / keep_rate.  keep_rate == 1 draws nothing
 * and philox_state may be null.  No atomics: sums over rows go through per-workgroup slabs in ws, added in a fixed order.
 * ws: sslrec_hyper_ws_bytes(N, n_split, d, K) bytes of device memory, contents irrelevant on entry, for either call. */
size_t sslrec_hyper_ws_bytes(int32_t N, int32_t n_split, int32_t d, int32_t K);

/* Y [N, d] = act(A act(A^T X)) per range.  H_u, H_i [d, K] receive act(A^T X) TRANSPOSED (element [j, k] = H[k, j]), which the
 * backward needs together with Y. */
int sslrec_hyper_fwd_f32(const float *X, const float *E, int32_t N, int32_t n_split, int32_t d, const float *W_u, const float *W_i, int32_t K,
                         float mult, float leaky, float keep_rate, const uint64_t *philox_state, uint32_t philox_stream, float *H_u,
                         float *H_i, float *Y, void *ws, void *stream);

/* From dY [N, d], the forward's Y, H_u, H_i and the SAME philox_state contents and philox_stream: dX, dE [N, d] (separate outputs: where
 * X and E are one tensor the caller adds them) and dW_u, dW_i [d, K] (zero for an empty range).  The slope of act comes from the sign
 * of Y and H; at exactly 0 it is `leaky`.  Two runs give the same bits. */
int sslrec_hyper_bwd_f32(const float *X, const float *E, const float *dY, const float *Y, int32_t N, int32_t n_split, int32_t d,
                         const float *W_u, const float *W_i, const float *H_u, const float *H_i, int32_t K, float mult, float leaky,
                         float keep_rate, const uint64_t *philox_state, uint32_t philox_stream, float *dX, float *dE, float *dW_u,
                         float *dW_i, void *ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * Graph-transformer layer of AutoCF / GFormer (csrc/gt.hip), GTLayer.forward of models/general_cf/autocf.py:109-129 (verbatim again in
 * gformer.py:221-255):
 *     qEmbeds = (embeds[rows] @ self.qTrans).view([-1, head_num, d // head_num])        (kEmbeds, vEmbeds from embeds[cols])
 *     att = t.clamp(t.einsum('ehd, ehd -> eh', qEmbeds, kEmbeds), -10.0, 10.0);  expAtt = t.exp(att)
 *     att = expAtt / (tem.index_add_(0, rows, expAtt)[rows] + 1e-8)
 *     resEmbeds = tem.index_add_(0, rows, t.einsum('eh, ehd -> ehd', att, vEmbeds).view([-1, d]))
 * with the projections hoisted to the nodes ((X[rows]) W = (X W)[rows]): Q, K, V [n, d] fp32 row-major are the projected NODE tables,
 * the pattern is square (n x n), WITHOUT duplicate entries, given as CSR (rowptr [n + 1], col [E]: column of every entry, rows in
 * order) and, for the backward, as CSC (colptr [n + 1], row [E]).  d in {32, 64, 128}, heads dividing d with d / heads in
 * {4, 8, 16, 32, 64, 128}.  long_rows / long_cols (n_long / n_long_cols of them, nullable when 0): the rows / columns of more than
 * SSLREC_EDGE_LONG_ROW entries, which get a workgroup each.  Nothing of size E x d or E x heads is written; no atomics, every sum in a
 * fixed order: two runs give the same bits.  SSLREC_E_BADARG before any launch for a null required pointer or a shape outside these
 * ranges; n == 0 returns 0 without a launch. */

/* Y [n, d] = sum over the row's entries of exp(clamp(<Q[r, h], K[c, h]>, -10, 10)) / (Z[r, h] + 1e-8) * V[c, h]; rows without entries are
 * exact zeros.  Z [n, heads] receives the row sums of the exponentials, which the backward needs together with Y. */
int sslrec_gt_fwd_f32(const int32_t *rowptr, const int32_t *col, int32_t n, const int32_t *long_rows, int32_t n_long, const float *Q,
                      const float *K, const float *V, int32_t d, int32_t heads, float *Y, float *Z, void *stream);

/* From dY [n, d] and the forward's Y, Z (autograd of the lines above): dQ, dK, dV [n, d], each nullable (not computed).  t_ws: n * heads
 * floats of device memory, contents irrelevant on entry (t[i, h] = <dY[i, h], Y[i, h]>, the row sums of a * da). */
int sslrec_gt_bwd_f32(const int32_t *rowptr, const int32_t *col, const int32_t *long_rows, int32_t n_long, const int32_t *colptr,
                      const int32_t *row, const int32_t *long_cols, int32_t n_long_cols, int32_t n, const float *Q, const float *K,
                      const float *V, const float *Y, const float *Z, const float *dY, int32_t d, int32_t heads, float *dQ, float *dK,
                      float *dV, float *t_ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * Alignment + uniformity loss of DirectAU (csrc/au.hip), models/loss_utils.py:75-86 at the call site models/general_cf/directau.py:42-47:
 *     anc_embeds = user_embeds[ancs];  pos_embeds = item_embeds[poss]
 *     align_loss = alignment(anc_embeds, pos_embeds)          x, y = F.normalize(x, dim=-1), F.normalize(y, dim=-1)
 *                                                              (x - y).norm(p=2, dim=1).pow(alpha).mean()                 (alpha = 2)
 *     uniform_loss = gamma * (uniformity(anc_embeds) + uniformity(pos_embeds)) / 2
 *                                                              t.pdist(F.normalize(x, dim=-1), p=2).pow(2).mul(-2).exp().mean().log()
 *     loss = align_loss + uniform_loss
 * on the stacked table T [N, d] fp32 row-major: row anc of the first n_user rows and row n_user + pos, both multiplied by `scale`
 * (directau.py:35 averages the layers: T is their SUM and scale = 1 / (L + 1)).  ancs, poss: int64 [B], duplicates welcome; an index
 * outside its part of the table contributes a zero row and receives no gradient.  d in {32, 64, 128}, 2 <= B <= 8192,
 * 0 <= n_user <= N, scale and gamma finite.  terms: bit 0 the alignment, bit 1 the uniformity of the anchors, bit 2 that of the
 * positives (1 .. 7; DirectAU: 7; a term left out is 0 in the sums above).  Nothing of size B x B or B (B - 1) / 2 is written; a pair
 * is left out when its two batch POSITIONS are equal, never by value; no float atomics, every sum in a fixed order: two runs give the
 * same bits.  SSLREC_E_BADARG before any launch for a null pointer or a value outside these ranges. */

/* bytes of the workspace both calls share (normalised rows, norms, per-split partial sums, staged gradient rows, scatter table);
 * 0 for arguments out of range */
size_t sslrec_au_ws_bytes(int32_t B, int32_t d);

/* out[0..2] = loss, align_loss, uniform_loss (directau.py:45-47); out[3..4] = the two sums over pairs, which the backward needs
 * (out: 8 floats of device memory).  ws: contents irrelevant on entry; the backward reads what this call leaves there. */
int sslrec_au_fwd_f32(const float *T, int32_t N, int32_t n_user, int32_t d, const int64_t *ancs, const int64_t *poss, int32_t B, float scale,
                      float gamma, int32_t terms, float *out, void *ws, void *stream);

/* Autograd of the lines above plus the index_put backward of both gathers (directau.py:43-44) in one call: with the SAME arguments,
 * `out` and `ws` as the forward left them, dT [N, d] (zero-initialised or already holding gradients) receives
 * g_align[0] * d align_loss / dT + g_uniform[0] * d uniform_loss / dT (device scalars; the same address for both is the gradient of
 * `loss`).  Rows that share a destination are added in ascending batch position. */
int sslrec_au_bwd_f32(int32_t N, int32_t n_user, int32_t d, const int64_t *ancs, const int64_t *poss, int32_t B, float scale, float gamma,
                      int32_t terms, const float *out, const float *g_align, const float *g_uniform, float *dT, void *ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * VGAE edge decoder of AdaGCL over all entries of a pattern (csrc/edgemlp.hip), models/general_cf/adagcl.py:221-237 (vgae_generate):
 *     edge_pred = self.sigmoid(self.decoder(x[edge_index[0]] * x[edge_index[1]]))       decoder = ReLU, Linear(d, d), ReLU, Linear(d, 1)
 *     mask = ((edge_pred + 0.5).floor()).type(t.bool)
 *     newVals = vals[mask];  newVals = newVals / (newVals.shape[0] / edgeNum[0]);  newIdxs = idxs[:, mask]
 * The pattern is given as the per-entry arrays of a plan's CSR (sslrec_sddmm_f32): row_of_entry, col, perm [nnz].  X [n, d] fp32
 * row-major serves both ends (the adjacency is square), W1 [d, d] row-major as nn.Linear stores it ([out, in]), b1 [d], w2 [d], b2 [1]
 * (device memory: no host round trip for a parameter).  d in {32, 64, 128}.  Forward only.  Nothing of size nnz x d is written; the
 * kept count is an integer sum: two runs give the same bits.  SSLREC_E_BADARG before any launch for a null pointer or a shape
 * outside these ranges. */

/* workgroups of the decoder launch at most = integers of its `counts` workspace */
#define SSLREC_EDGE_MLP_SLOTS 1024

/* logit[perm[k]] = w2 . relu(W1 relu(X[row] (.) X[col]) + b1) + b2 and keep[perm[k]] = logit >= 0 for every CSR position k.  The
 * reference's floor(sigmoid(logit) + 0.5) differs from this flag only for fp32 logits within a few 2^-23 below 0, where the fp32
 * sigmoid already rounds to 0.5.  counts [SSLREC_EDGE_MLP_SLOTS]: kept entries per workgroup, *n_counts (host) how many were written. */
int sslrec_edge_mlp_fwd_f32(const int32_t *row_of_entry, const int32_t *col, const int32_t *perm, int32_t n_rows, int32_t n_cols, int32_t nnz,
                            const float *X, int32_t d, const float *W1, const float *b1, const float *w2, const float *b2, float *logit,
                            uint8_t *keep, int32_t *counts, int32_t *n_counts, void *stream);

/* the same flags and counts from logits that something else computed (an embedding size without a decoder kernel) */
int sslrec_edge_keep_flags(const float *logit, int32_t nnz, uint8_t *keep, int32_t *counts, int32_t *n_counts, void *stream);

/* The finishing launch (:232-234): kept[0] = sum of the counts, out[e] = keep[e] ? vals[e] / (float)(kept / nnz) : 0 in entry order --
 * the values of a re-valued view of the SAME plan, dropped entries 0.  kept == 0 writes zeros everywhere (no division by 0). */
int sslrec_edge_keep_finish_f32(const float *vals, const uint8_t *keep, const int32_t *counts, int32_t n_counts, int32_t nnz, float *out,
                                int32_t *kept, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * DenoiseNet's edge gate and symmetric normalisation of AdaGCL (csrc/gate.hip), models/general_cf/adagcl.py:274-338, :358-401, :340-347:
 *     weight = self.get_attention(x[self.row], x[self.col], layer)              (Linear + ReLU per end, concat, Linear(2 d, 1))
 *     gate_inputs = t.sigmoid((t.log(u) - t.log(1 - u) + log_alpha) / beta)     (training; t.sigmoid(log_alpha) otherwise)
 *     mask = t.clamp(gate_inputs * (zeta - gamma) + gamma, 0.0, 1.0)
 *     rowsum = t.sparse.sum(adj, dim=-1).to_dense() + 1e-6;  d_inv_sqrt = t.clamp(t.pow(rowsum, -0.5), 0.0, 10.0)
 *     values = mask * d_inv_sqrt[row] * d_inv_sqrt[col]
 *     l0_norm = t.mean(t.sigmoid(log_alpha - beta * t.log(-gamma / zeta)))
 * with log_alpha[e] = p[row(e)] + q[col(e)] + bias[0]: the Linear + ReLU of the gathered rows is the gather of the transformed node
 * table and the last Linear splits into two dots, so p, q [n] are node vectors.  The pattern is square (n x n), given as the plan's
 * CSR (rowptr [n + 1], col, perm, row_of_entry [nnz]) and, for the backward, the transposed plan's (rowptr_t, col_t, perm_t);
 * long_rows / long_rows_t: rows of more than SSLREC_EDGE_LONG_ROW entries (nullable when 0).  noise [nnz] in entry order = the
 * logistic noise log u - log(1 - u), or null: then the gate's input is log_alpha itself (beta enters l0 only).  gamma < 0 < zeta,
 * beta > 0, eps >= 0.  The ROW sums serve both ends, as in the reference.  No float atomics, every sum in a fixed order. */

/* m [nnz] the clamped gates, s [n] = eps + their row sums, dinv [n], vals [nnz], l0 [1]; l0_row: n floats of workspace */
int sslrec_edge_gate_fwd_f32(const int32_t *rowptr, const int32_t *col, const int32_t *perm, const int32_t *row_of_entry, int32_t n, int32_t nnz,
                             const int32_t *long_rows, int32_t n_long, const float *p, const float *q, const float *bias, const float *noise,
                             float gamma, float zeta, float beta, float eps, float *m, float *s, float *dinv, float *vals, float *l0,
                             float *l0_row, void *stream);

/* From dvals [nnz], dl0 [1] and the forward's m, s, dinv: dp, dq [n], dbias [1].  The gradient is 0 where the clamp at 10 or the
 * [0, 1] clamp is active.  dla_ws: nnz floats, n_ws: 2 n floats of workspace, contents irrelevant on entry. */
int sslrec_edge_gate_bwd_f32(const int32_t *rowptr, const int32_t *col, const int32_t *perm, const int32_t *long_rows, int32_t n_long,
                             const int32_t *rowptr_t, const int32_t *col_t, const int32_t *perm_t, const int32_t *long_rows_t, int32_t n_long_t,
                             int32_t n, int32_t nnz, const float *p, const float *q, const float *bias, const float *noise, float gamma,
                             float zeta, float beta, float eps, const float *m, const float *s, const float *dinv, const float *dvals,
                             const float *dl0, float *dp, float *dq, float *dbias, float *dla_ws, float *n_ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * Lloyd's k-means of NCL (csrc/kmeans.hip), the loop of KMeansClustering.forward, models/aug_utils.py:149-156:
 *     for i in range(1000):
 *         dists = (embeds.view([-1, 1, d]) - centroids.view([1, -1, d])).square().sum(-1)
 *         _, idxs = t.min(dists, dim=1)
 *         newCents = t.zeros_like(centroids);  newCents.index_add_(0, idxs, embeds)
 *         clustNums = t.zeros([K, 1]);         clustNums.index_add_(0, idxs, ones)
 *         centroids = newCents / (clustNums + 1e-6)
 * on X [N, d] fp32 row-major, N >= 1, d in {32, 64, 128}, K >= 1 with K * d * 4 <= 64 KiB.  Nothing of size N x K is written.  Distances
 * in the difference form in fp32; among equal distances the LOWEST cluster index wins; no float atomics, every sum in an order that
 * depends on (N, K, d) and idx only: two runs give the same bits.  An empty cluster gets the centroid 0 and the count 0.
 * SSLREC_E_BADARG before any launch for a null pointer, a value outside these ranges, or X / cent not 16-byte aligned. */

/* bytes of the workspace (slab partial sums and counts, changed-row counters); 0 for arguments out of range */
size_t sslrec_kmeans_ws_bytes(int32_t N, int32_t K, int32_t d);

/* cent [K, d]: the initial centroids on entry (t.rand([K, d]), :147), the final ones on return; idx [N] int32 and counts [K] (the
 * integer cluster sizes as fp32, clustNums) are written.  Runs max_iter >= 1 iterations of three launches each on `stream`.  early_exit
 * != 0: every `poll` (1 .. 64) iterations the host reads how many rows changed their cluster in each of them (one copy, one stream
 * synchronisation) and stops after the first period in which some iteration changed none -- every further iteration would reproduce
 * centroids, idx and counts bit for bit, so the result is that of max_iter iterations.  iters_run[0] (host memory) = iterations
 * launched.  early_exit == 0: no copy, no synchronisation.  Not capturable into a hipGraph with early_exit. */
int sslrec_kmeans_f32(const float *X, int32_t N, int32_t d, int32_t K, float *cent, int32_t *idx, float *counts, int32_t max_iter,
                      int32_t early_exit, int32_t poll, int32_t *iters_run, void *ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * GFormer's anchor distances (csrc/bfs.hip), get_random_anchorset of models/general_cf/gformer.py:152-176:
 *     graph = nx.Graph();  graph.add_edges_from(zip(rows, cols))
 *     dicts_dict[node] = nx.single_source_shortest_path_length(graph, node, cutoff=None)       for every anchor
 *     dists_array[i, j] = 1 / (dist + 1)                                                        in a Python double loop
 * as one level-synchronous multi-source BFS with a 64-bit reached mask per node and 64 anchors, pull form, over the CSR of the pattern
 * (rowptr [n + 1], col [E], n x n, SYMMETRIC -- not checked; duplicate entries are harmless).  long_rows: the rows of more than
 * SSLREC_EDGE_LONG_ROW entries (nullable when n_long = 0), which get a workgroup each.  1 <= A <= 256, 1 <= n < 2^31; anchors [A] int32,
 * distinct.  hops [n, A] int16 row-major: the hop count of node n from anchor a, 0 for the anchor itself, -1 for an unreached node; the
 * reference's weight is hop < 0 ? 0 : 1 / (hop + 1).  Integers only: exact, and two runs give the same bits.
 * SSLREC_E_BADARG before any launch for a null pointer or a value outside these ranges. */

/* bytes of the workspace (two reached buffers, the per-level counters); 0 for arguments out of range */
size_t sslrec_anchor_hops_ws_bytes(int32_t n, int32_t A);

/* Every `poll` (1 .. 64) levels the host reads how many rows gained a bit in each of them (one copy, one stream synchronisation) and
 * stops after the first period in which some level changed nothing; later levels are the identity, so the result does not depend on
 * `poll`.  levels[0] (host) = the levels that changed something, converged[0] (host) = 1 -- or, when 32766 levels have all changed
 * something, converged[0] = 0: the caller must treat that as an error (int16 would be exceeded next), nothing saturates silently. */
int sslrec_anchor_hops(const int32_t *rowptr, const int32_t *col, int32_t n, const int32_t *long_rows, int32_t n_long, const int32_t *anchors,
                       int32_t A, int16_t *hops, int32_t poll, int32_t *levels, int32_t *converged, void *ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * GFormer's position features (csrc/pnn.hip), PNNLayer.forward of models/general_cf/gformer.py:202-218:
 *     set_ids_reshape = embeds[anchor_set_id].repeat(N, 1).reshape(-1, A, d);  messages = set_ids_reshape * dists_array.T.unsqueeze(2)
 *     self_feature = embeds.repeat(A, 1).reshape(-1, A, d)
 *     outposition1 = t.mean(self.linear_hidden(t.cat((messages, self_feature), dim=-1)), dim=1)
 * with the Linear commuted past the mean: Z [N, 2d] = [s, u], s[n] = (1 / A) sum_a w[n, a] X[anchors[a]] with w decoded from hops
 * (sslrec_anchor_hops), u[n] = (1 / A) sum_{a < A} X[(n A + a) mod N] -- element [n, a] of the reference's self_feature is that row, not
 * row n.  The caller applies the Linear.  X [N, d] fp32 row-major, 16-byte aligned; d in {32, 64, 128}, 1 <= A <= 256, A d 4 <= 128 KiB,
 * 1 <= N < 2^31; anchors [A] int32 in [0, N) (distinct in the model; a repeated id is handled exactly); hops [N, A] int16.  Nothing of size N x A x d or N x A floats is written, no
 * float atomics, every sum in a fixed order.  SSLREC_E_BADARG before any launch for a null pointer or a shape outside these ranges.  The ids live on
 * the device and are NOT checked: an id outside [0, N) gives an undefined result (forward and backward), no error code; no memory outside
 * the tables is touched. */
int sslrec_pnn_fwd_f32(const float *X, int32_t N, int32_t d, const int32_t *anchors, int32_t A, const int16_t *hops, float *Z, void *stream);

/* bytes of the backward's workspace (slab partial sums of the anchor rows' gradient and their total); 0 for shapes out of range */
size_t sslrec_pnn_bwd_ws_bytes(int32_t N, int32_t A, int32_t d);

/* dX [N, d] (written, not added to) from gZ [N, 2d]: the window half as a gather, dX[m] = (1 / A) sum_{j < A} gu[(m + j N) / A], then
 * dX[anchors[a]] += (1 / A) sum_n w[n, a] gs[n]. */
int sslrec_pnn_bwd_f32(const float *gZ, int32_t N, int32_t d, const int32_t *anchors, int32_t A, const int16_t *hops, float *dX, void *ws,
                       void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * Per-entry attention of GFormer's LocalGraph (csrc/gt.hip), models/general_cf/gformer.py:235-255 with :351-352:
 *     embeds_l2, atten = self.gt_layer(add_adj, embeds);  att_edge = t.sum(atten, dim=-1)
 * out[k] = sum_h exp(clamp(<Q[r, h], K[c, h]>, -10, 10)) / (Z[r, h] + 1e-8) for every CSR position k = (r, c) of the pattern; arguments
 * and shapes as sslrec_gt_fwd_f32.  Forward only.  z_ws: n * heads floats (sslrec_gt_scores_ws_bytes; 0 for a shape without a kernel). */
size_t sslrec_gt_scores_ws_bytes(int32_t n, int32_t d, int32_t heads);
int sslrec_gt_scores_f32(const int32_t *rowptr, const int32_t *col, int32_t n, const int32_t *long_rows, int32_t n_long, const float *Q,
                         const float *K, int32_t d, int32_t heads, float *out, float *z_ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * MHCN's row-wise kernels (csrc/mhcn.hip), models/social/mhcn.py.  Tables are [N, d] fp32 row-major, 16-byte aligned, d in {32, 64, 128},
 * 1 <= N < 2^31.  No float atomics; every sum over rows is formed from per-workgroup partials in a fixed order, so two calls give the
 * same bits.  SSLREC_E_BADARG before any launch for a null pointer, a misaligned table or a shape outside these ranges.
 *
 * Self-gating units (csrc/mhcn_gate.hip), mhcn.py:34-52:  gates = t.sigmoid(self.gatingC(em));  return em * gates
 * for C <= 4 gates sharing one table: Y_c = X (.) sigmoid(X W_c^T + b_c) in ONE launch on the exact-fp32 MFMA.  Wt [C, d, d]: the
 * TRANSPOSED weights, Wt[c][i][k] = W_c[k][i] for nn.Linear's out x in weight W_c; B [C, d] the biases (16-byte aligned); Y0 .. Y3: the C
 * outputs (the others may be null).  Nothing but the outputs is written: the backward recomputes the logits. */
int sslrec_mhcn_gate_fwd_f32(const float *X, int32_t N, int32_t d, const float *Wt, const float *B, int32_t C, float *Y0, float *Y1, float *Y2,
                             float *Y3, void *stream);

/* bytes of the backward's workspace: per gate and workgroup one [d, d] slab of dW^T and one [d] partial of db; 0 for a shape out of range */
size_t sslrec_mhcn_gate_ws_bytes(int32_t N, int32_t d, int32_t C);

/* From dY0 .. dY3 [N, d]: dX [N, d] = sum_c (dY_c (.) s_c + T_c W_c) with s_c the gate and T_c = dY_c (.) X (.) s_c (1 - s_c), dW [C, d, d]
 * with dW[c] = T_c^T X in nn.Linear's out x in layout (NOT transposed), dB [C, d] the column sums of T_c.  All three are written. */
int sslrec_mhcn_gate_bwd_f32(const float *X, int32_t N, int32_t d, const float *Wt, const float *B, int32_t C, const float *dY0, const float *dY1,
                             const float *dY2, const float *dY3, float *dX, float *dW, float *dB, void *ws, void *stream);

/* Workspace of the backward of the channel mix and of both directions of the loss: per-workgroup column partials and their total; 0 for
 * a shape without a kernel. */
size_t sslrec_mhcn_ws_bytes(int32_t N, int32_t d);

/* Channel attention with the normalised layer sums, mhcn.py:54-64 as :81 and :112-113 call it, with :84-101:
 *     weight_c = (attn * (embed_c @ attn_mat)).sum(1);  score = softmax over the three channels;  mixed = sum_c score_c embed_c
 *     mixed_embed = mixed + simp_user_embeds / 2;       all_embeds_k += [F.normalize(embeds_k, p=2, dim=1)]
 * v [d] = attn_mat @ attn^T is formed by the caller, weight_c = <embed_c, v>.  mixed [N, d] and scores [N, 3] are written; with
 * a1 .. a4 (all four or none) also o_k = a_k + e_k / max(|e_k|, 1e-12) for e = (c1, c2, c3, simp), o_k may alias a_k. */
int sslrec_mhcn_mix_fwd_f32(const float *c1, const float *c2, const float *c3, const float *simp, const float *v, int32_t N, int32_t d,
                            const float *a1, const float *a2, const float *a3, const float *a4, float *mixed, float *scores, float *o1, float *o2,
                            float *o3, float *o4, void *stream);

/* Its backward from g_mixed [N, d] and, if given (all four or none), the gradients go_k of o_k: d1, d2, d3, dsimp [N, d] and dv [d] are
 * written.  A row with |e_k| < 1e-12 receives go_k / 1e-12, the clamp's gradient.  scores: what the forward wrote.  The gradient in a_k
 * is go_k itself and is not written. */
int sslrec_mhcn_mix_bwd_f32(const float *c1, const float *c2, const float *c3, const float *simp, const float *v, const float *scores, int32_t N,
                            int32_t d, const float *g_mixed, const float *go1, const float *go2, const float *go3, const float *go4, float *d1,
                            float *d2, float *d3, float *dsimp, float *dv, void *ws, void *stream);

/* The same sum for one table (the item side, mhcn.py:95-97): out = acc + x / max(|x|, 1e-12); dx from the gradient g of out. */
int sslrec_mhcn_normadd_fwd_f32(const float *acc, const float *x, int32_t N, int32_t d, float *out, void *stream);
int sslrec_mhcn_normadd_bwd_f32(const float *x, const float *g, int32_t N, int32_t d, float *dx, void *stream);

/* Hierarchical mutual-information loss, mhcn.py:121-143 with edge = adj @ em formed by the caller:
 *     pos = score(em, edge);  neg1 = score(row_shuffle(em), edge);  neg2 = score(row_col_shuffle(edge), em)
 *     local = -((pos - neg1).sigmoid().log() + (neg1 - neg2).sigmoid().log()).sum()
 *     graph = edge.mean(0);  global = -(score(edge, graph) - score(row_col_shuffle(edge), graph)).sigmoid().log().sum()
 * The shuffles are given as int32 permutations: row_shuffle(x) = x[row_u], the two row_col_shuffle(x) = x[row_k][:, col_k] (k = 1 for
 * neg2, k = 2 for the global term).  log sigmoid(x) is computed as min(x, 0) - log1p(exp(-|x|)): equal to the reference wherever that is
 * finite, and finite where it returns -inf.  The loss is accumulated in double.  Written: loss [1], graph [d] and coef [N, 3], the three
 * sigmoid(-x) per row, which the backward reads.  An index outside its range reads row / column 0: an undefined result, no error. */
int sslrec_mhcn_ssl_fwd_f32(const float *em, const float *edge, const int32_t *row_u, const int32_t *col_1, const int32_t *row_1,
                            const int32_t *col_2, const int32_t *row_2, int32_t N, int32_t d, float *coef, float *graph, float *loss, void *ws,
                            void *stream);

/* d_em, d_edge [N, d] (written) for the upstream gradient gloss [1] on the device.  inv_*: the inverse permutations (inv[p[i]] = i): every
 * scatter through a permutation is a gather through its inverse.  No [N, d] shuffled copy exists in either direction. */
int sslrec_mhcn_ssl_bwd_f32(const float *em, const float *edge, const int32_t *row_u, const int32_t *col_1, const int32_t *row_1,
                            const int32_t *col_2, const int32_t *row_2, const int32_t *inv_row_u, const int32_t *inv_col_1,
                            const int32_t *inv_row_1, const int32_t *inv_col_2, const int32_t *inv_row_2, const float *coef, const float *graph,
                            const float *gloss, int32_t N, int32_t d, float *d_em, float *d_edge, void *ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * KGIN's kernels (csrc/kgin.hip), models/kg/kgin.py.  Tables are [*, d] fp32 row-major, 16-byte aligned, d in {32, 64, 128}.  No float
 * atomics; two calls give the same bits.  SSLREC_E_BADARG before any launch for a null pointer, a misaligned table or a shape outside
 * these ranges.
 *
 * An EDGE LIST in some order (graph.RelGraph builds one by head, one by tail and one by relation): ptr [n_dest + 1] int32 and per slot
 * ia, ib (the rows of the two tables that the slot multiplies) and eid (the edge's id in the caller's numbering: keep [E] uint8, or
 * null, is read through it).  A destination of more than SSLREC_KGIN_CHUNK slots is LONG: chunk_dest / chunk_begin [n_chunks] list its
 * chunks (all chunks of one destination in a row, in slot order), long_dest [n_long] / long_ptr [n_long + 1] its range of chunks;
 * part [n_chunks, d] (and part_cnt [n_chunks] int32 forward) take the chunks' sums, which a second launch adds in chunk order.  The
 * index arrays must hold valid rows: the kernels do not check them.
 *
 * Relational aggregation, kgin.py:33-36:
 *     edge_relation_emb = weight[edge_type - 1];  neigh_relation_emb = entity_emb[tail] * edge_relation_emb
 *     entity_agg = scatter_mean(src=neigh_relation_emb, index=head, dim_size=n_entities, dim=0)
 * on the list ordered by head (ia = tail, ib = relation): Y [n_dest, d] and cnt [n_dest], the integer number of kept edges of every head
 * (the mean of no edge is 0).  W [R, d] sits in LDS when it fits 48 KiB. */
#define SSLREC_KGIN_CHUNK 512
int sslrec_kgin_rel_fwd_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                            const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                            const int32_t *long_ptr, int32_t n_long, const float *X, const float *W, int32_t R, int32_t d, const uint8_t *keep,
                            int32_t *cnt, float *Y, float *part, int32_t *part_cnt, void *stream);

/* The backward of the same lines, one call per gradient: out[dest] = sum over the kept slots of G[ia] (.) B[ib] / max(cnt[ia], 1) with
 * ia = head in both.  dX: the list ordered by tail, B = W [R, d] (b_in_lds = 1: staged in LDS when it fits), ib = relation.
 * dW: the list ordered by relation, B = X, ib = tail (b_in_lds = 0).  cnt: what the forward wrote. */
int sslrec_kgin_rel_bwd_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                            const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                            const int32_t *long_ptr, int32_t n_long, const float *G, const float *B, int32_t n_b_rows, int32_t b_in_lds, int32_t d,
                            const uint8_t *keep, const int32_t *cnt, float *out, float *part, void *stream);

/* Factor modulation of the user side, kgin.py:38-46:
 *     score = softmax(user_emb @ latent_emb.t(), dim=1);  disen_weight = softmax(disen_weight_att, -1) @ weight
 *     user_agg = user_agg * (disen_weight.expand(U, F, d) * score.unsqueeze(-1)).sum(dim=1) + user_agg
 * out = agg (.) (p @ Dm) + agg per row with p = softmax_f <u, latent_f>; latent, Dm [F, d], 1 <= F <= 8, Dm = disen_weight formed by the
 * caller.  One launch, no [U, F, d] tensor. */
int sslrec_kgin_fm_fwd_f32(const float *agg, const float *u, const float *latent, const float *Dm, int32_t U, int32_t d, int32_t F, float *out,
                           void *stream);

/* bytes of the backward's workspace (per workgroup one [2 F, d] slab); 0 for a shape without a kernel */
size_t sslrec_kgin_fm_ws_bytes(int32_t U, int32_t d, int32_t F);

/* Its backward from gout [U, d]: d_agg, d_u [U, d] and d_latent_and_d [2 F, d] (dlatent, then dDm) are written; the softmax is
 * recomputed, the two [F, d] sums over rows come from per-workgroup slabs added in a fixed order by a finishing launch. */
int sslrec_kgin_fm_bwd_f32(const float *agg, const float *u, const float *latent, const float *Dm, const float *gout, int32_t U, int32_t d, int32_t F,
                           float *d_agg, float *d_u, float *d_latent_and_d, void *ws, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * KGCL's relation-aware graph attention (csrc/rgat.hip), models/kg/kgcl.py.  Tables are [*, d] fp32 row-major, 16-byte aligned, d in
 * {32, 64, 128}; slope >= 0.  The edge lists are those of the KGIN entries above (one order of a graph.RelGraph each, chunks of
 * SSLREC_KGIN_CHUNK slots for the long destinations, `keep` read through eid, NULL = every edge).  No float atomics; two calls give the
 * same bits.  SSLREC_E_BADARG before any launch for a null pointer, a misaligned table or a shape outside these ranges.
 *
 * Forward, kgcl.py:60-72 (RGAT.agg):
 *     a_input = cat([entity_emb[head], entity_emb[tail]], -1);  e_input = (fc(a_input) * relation_emb[edge_type]).sum(-1)
 *     e = scatter_softmax(leakyrelu(e_input), head);  agg_emb = scatter_sum(entity_emb[tail] * e.view(-1, 1), head)
 * with fc(cat(x[h], x[t])) = P[h] + Q[t], the node tables P = X Wh^T + b and Q = X Wt^T formed by the caller.  The list ordered by head
 * (ia = tail, ib = relation).  Written: Y [n_dest, d]; S [E] by EDGE ID, the logit after the LeakyReLU of every kept edge (other entries
 * are left alone); M, Z [n_dest], the maximum and the sum of exp(S - M) over the head's kept edges (Z = 0, M = 0, Y = 0 for a head
 * without one).  part [n_chunks, d] and part_mz [n_chunks, 2] take the chunks' (acc, m, z), merged in chunk order by a second launch.
 * R [n_rel, d] sits in LDS when it fits 48 KiB. */
int sslrec_rgat_fwd_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                        const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr,
                        int32_t n_long, const float *X, const float *P, const float *Q, const float *R, int32_t n_rel, int32_t d, float slope,
                        const uint8_t *keep, float *S, float *M, float *Z, float *Y, float *part, float *part_mz, void *stream);

/* The backward of the same lines (what autograd derives from scatter_softmax / scatter_sum / the two gathers), three walks from G = dY.
 * By head (the forward's list): alpha [E] and dl [E] by edge id for the kept edges, alpha_e = exp(S_e - M_h) / Z_h,
 * dl_e = alpha_e (<G[h], X[t]> - <G[h], Y[h]>) (S_e > 0 ? 1 : slope), and dP[h] = sum dl_e R[r].  part [n_chunks, d]. */
int sslrec_rgat_bwd_head_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                             const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                             const int32_t *long_ptr, int32_t n_long, const float *X, const float *R, int32_t n_rel, int32_t d, float slope,
                             const uint8_t *keep, const float *G, const float *Y, const float *S, const float *M, const float *Z, float *alpha,
                             float *dl, float *dP, float *part, void *stream);

/* By tail (ia = head, ib = relation): dX[t] = sum alpha_e G[h] and dQ[t] = sum dl_e R[r] in one walk.  part [n_chunks, 2, d]. */
int sslrec_rgat_bwd_tail_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                             const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                             const int32_t *long_ptr, int32_t n_long, const float *G, const float *R, int32_t n_rel, int32_t d, const uint8_t *keep,
                             const float *alpha, const float *dl, float *dX, float *dQ, float *part, void *stream);

/* By relation (ia = head, ib = tail): dR[r] = sum dl_e (P[h] + Q[t]).  part [n_chunks, d]. */
int sslrec_rgat_bwd_rel_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                            const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                            const int32_t *long_ptr, int32_t n_long, const float *P, const float *Q, int32_t d, const uint8_t *keep, const float *dl,
                            float *dR, float *part, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------------------
 * KGRec's two-head relational attention (csrc/rmha.hip), models/kg/kgrec.py.  Tables are [*, d] fp32 row-major, 16-byte aligned, d in
 * {32, 64, 128}, exactly two attention heads: head a owns the columns [a d/2, (a + 1) d/2), c = 1 / sqrt(d / 2).  The edge lists are
 * those of the KGIN entries above (one order of a graph.RelGraph each, chunks of SSLREC_KGIN_CHUNK slots for the long destinations,
 * `keep` read through eid, NULL = every edge).  No float atomics; two calls give the same bits.  SSLREC_E_BADARG before any launch for
 * a null pointer, a misaligned table or a shape outside these ranges.
 *
 * Forward, kgrec.py:63-82 (AttnHGCN.shared_layer_agg):
 *     query = (entity_emb[head] @ W_Q).view(-1, 2, d_k);  key = (entity_emb[tail] @ W_Q).view(-1, 2, d_k) * relation_emb[edge_type - 1]
 *     edge_attn_score = scatter_softmax((query * key).sum(-1) / sqrt(d_k), head)
 *     entity_agg = scatter_sum((entity_emb[tail] * relation_emb[edge_type - 1]).view(-1, 2, d_k) * edge_attn_score, head)
 * with the node table T = X W_Q formed by the caller.  The list ordered by head (ia = tail, ib = relation).  Written: Y [n_dest, d];
 * Lg [E, 2] by EDGE ID, the two logits of every kept edge (other entries are left alone); M, Z [n_dest, 2], the maximum and the sum of
 * exp(Lg - M) over the head entity's kept edges per attention head (Z = 0, M = 0, Y = 0 without one).  part [n_chunks, d] and part_mz
 * [n_chunks, 2, 2] take the chunks' acc and (m, z) per attention head, merged in chunk order by a second launch.  R [n_rel, d] sits in
 * LDS when it fits 48 KiB. */
int sslrec_rmha_fwd_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                        const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr,
                        int32_t n_long, const float *X, const float *T, const float *R, int32_t n_rel, int32_t d, const uint8_t *keep, float *Lg,
                        float *M, float *Z, float *Y, float *part, float *part_mz, void *stream);

/* The backward of the same lines (what autograd derives from the softmax, the scatter_sum and the gathers), three walks from G = dY.
 * By head (the forward's list): alpha [E, 2] and dl [E, 2] by edge id for the kept edges, alpha_ea = exp(Lg_ea - M_ha) / Z_ha,
 * dl_ea = alpha_ea (sum_{C_a} G[h] X[t] R[r] - sum_{C_a} G[h] Y[h]), and dT[h] = c sum dl_ea T[t] R[r].  part [n_chunks, d]. */
int sslrec_rmha_bwd_head_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                             const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                             const int32_t *long_ptr, int32_t n_long, const float *X, const float *T, const float *R, int32_t n_rel, int32_t d,
                             const uint8_t *keep, const float *G, const float *Y, const float *Lg, const float *M, const float *Z, float *alpha,
                             float *dl, float *dT, float *part, void *stream);

/* By tail (ia = head, ib = relation): dX[t] = sum alpha_ea G[h] R[r] and dT[t] = c sum dl_ea T[h] R[r] in one walk (the caller adds the
 * two halves of dT).  part [n_chunks, 2, d]. */
int sslrec_rmha_bwd_tail_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                             const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                             const int32_t *long_ptr, int32_t n_long, const float *G, const float *T, const float *R, int32_t n_rel, int32_t d,
                             const uint8_t *keep, const float *alpha, const float *dl, float *dX, float *dT, float *part, void *stream);

/* By relation (ia = head, ib = tail): dR[r] = sum (c dl_ea T[h] T[t] + alpha_ea G[h] X[t]).  part [n_chunks, d]. */
int sslrec_rmha_bwd_rel_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                            const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                            const int32_t *long_ptr, int32_t n_long, const float *G, const float *X, const float *T, int32_t d, const uint8_t *keep,
                            const float *alpha, const float *dl, float *dR, float *part, void *stream);

/* The rationale scores, kgrec.py:165-188 (norm_attn_computer, under no_grad), on the list ordered by head:
 *     edge_attn_logits = ((query * key).sum(-1) / sqrt(d_k)).mean(-1);  edge_attn_score = scatter_softmax(edge_attn_logits, head) * degree[head]
 * logit, score [E] by edge id for the kept edges (the caller zeroes both first); mean_head [n_dest], the mean of the scores over the head
 * entity's kept edges, 0 without one (the scatter_mean of kgrec.py:414), evaluated as Z (count / Z) / count: the scores of one entity add
 * up to (count / Z) sum exp(l - M).  part_mz [n_chunks, 2], part_cnt [n_chunks]. */
int sslrec_rmha_score_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                          const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                          const int32_t *long_ptr, int32_t n_long, const float *T, const float *R, int32_t n_rel, int32_t d, const uint8_t *keep,
                          float *logit, float *score, float *mean_head, float *part_mz, int32_t *part_cnt, void *stream);

/* mean [n_dest]: the mean of score (by edge id) over the kept slots of every destination of a list, 0 without one; on the list ordered
 * by tail the scatter_mean of kgrec.py:416.  part_sum, part_cnt [n_chunks]. */
int sslrec_rmha_mean_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                         const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr,
                         int32_t n_long, const uint8_t *keep, const float *score, float *mean, float *part_sum, int32_t *part_cnt, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSLREC_HIP_H */
