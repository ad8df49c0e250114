/*
 * aabr_hip.h -- C ABI of libaabr_hip.so, the MI355X (gfx950) implementation of the
 * sparse-3D detection hot path of xuyongzhi/Automatic-As-built-Reconstruction:
 * voxel scatter -> hash grid -> rule tables -> sparse conv (MFMA) -> BN -> rotated IoU/NMS.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless its name ends in `_host`;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *    synchronises unless stated;
 *  - every entry point returns 0 on success or a negative AABR_E* code;
 *    aabr_last_error() returns a static message for the calling thread;
 *  - row-major, contiguous arrays; features are float32 [rows, planes];
 *    site coordinates are int32 [rows,4] = (x, y, z, batch); rule tables are
 *    int32 [filter_volume][rows] "gather tables" (entry = partner row, or -1).
 *
 * The reference binds this path through two pybind11 extension modules
 * (SparseConvNet/sparseconvnet/SCN/pybind.cpp:11-235 `sparseconvnet.SCN`,
 *  maskrcnn_benchmark/csrc/vision.cpp:9-20 `_C`) whose arguments are at::Tensor /
 * Metadata<3>&.  Each function below cites the reference interface it replaces;
 * INTEGRATION.md shows the ctypes binding that reproduces the reference names.
 */
#ifndef AABR_HIP_H
#define AABR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AABR_OK 0
#define AABR_EINVAL (-1)  /* bad argument (null pointer, negative size, unsupported shape) */
#define AABR_ELAUNCH (-2) /* HIP launch / runtime error */
#define AABR_ERANGE (-3)  /* coordinate outside the supported [0, 65534] range */

const char *aabr_last_error(void);
/* ABI version: bumped whenever a signature, a record layout or AABR_META_WORDS changes; a binding written for one value
 * must refuse a library that reports another (`_hip.load()` does).  500 = round 5 (16-word meta blocks, brick grids);
 * 600 = round 6 (regression targets out of the label kernel, list encode / decode, fused small-map records);
 * 610 = the RPN loss (aabr_rpn_loss_*, aabr_sample_list, aabr_smooth_l1_*); 620 = the ROI box post-processor
 * (aabr_roi_post_*); 630 = aabr_roi_align_rotated_3d_forward_batch (the dense ROI-align forward told the batch size);
 * 640 = the box head's loss (aabr_roi_targets, aabr_roi_box_loss_*).
 * The multi-level ROI pooler (aabr_roi_pool_*, AabrRoiLevel) came after 640 WITHOUT a bump: it adds symbols and one new
 * record only, no existing signature or layout changed, so a binding written for 640 still matches.  The box head's
 * dense layers (aabr_roi_mlp_*) and the RPN head (aabr_rpn_head_*, AabrRpnMap) came the same way: symbols only.  So did
 * the deferred-join tail of a launch plan (AABR_PLAN_TAIL, AABR_PLAN_TAIL_JOIN, aabr_plan_run_tail, aabr_plan_tail_*):
 * one flag bit and one record kind that no earlier list carries, four new symbols, AabrPlanOp unchanged.  The corner
 * form of the box coder (aabr_box_to_2corners, aabr_box_from_2corners, aabr_box_encode_corner, aabr_box_decode_corner,
 * aabr_roi_targets_coder, aabr_roi_post_detections_coder) likewise: six new symbols, the older entry points being the
 * centroid case of the same code; and fc6 over windows of the convolution rows (aabr_roi_mlp_*_window, AabrMlpWindow):
 * three new symbols and one new record.  The RPN with separated-classifier groups (aabr_rpn_head_grouped_*,
 * aabr_rpn_loss_grouped_*): six new symbols; the plain entry points run the same kernels and give the same bits.  The batched
 * input layer (aabr_bl_input_layer_sites, aabr_bl_points_prepare, aabr_quantize_scenes_bl): three new symbols; the flat
 * entry points run the same kernel bodies through the flat reader and give the same bits.  bf16 storage of the pooled ROI
 * tensor and its gradient (aabr_roi_pool_*_pooled_bf16, aabr_roi_mlp_*_pooled_bf16): five new symbols, AabrRoiLevel
 * unchanged; the fp32 entry points run the instances they ran before. */
#define AABR_ABI_VERSION 640
int aabr_version(void);
/* Tuning knobs for experiments and tests (no counterpart in the reference; the defaults are what ships): CONV_WIDE,
 * CONV_WIDE_BF16 (0 = never / 1 = whenever supported), WIDE_ROWS, WIDE_NBUF, CONV_WLDS,
 * CONV_SMALL, CONV_NBW, CONV_WPB, VOXEL_MEAN, GEOM_JOBS (0: aabr_geom_run issues its stream builders book by book), WIDE_XOFF
 * (0: k_conv_cs never lets a step straddle a filter offset; otherwise, the default, its fp32 instances of up to 64 input
 * channels step over the tile's block list: same bits).  PLAN_TAIL
 * (0 / 1 / 2: where AABR_PLAN_TAIL records run, see the compiled launch plans below; 2 ships).  A knob takes its value from the environment variable AABR_<NAME>,
 * read ONCE at its first use in the process; aabr_set_knob overrides it (unset != 0: back to "no value").  No entry
 * point reads the environment on its launch path.                                                              */
int aabr_set_knob(const char *name, int value, int unset);
/* bit 0: a `make DEV=1` build -- it additionally carries the phase-clock variants of k_conv_cs that tools/tools_cs_phases.py
 * reads (flags >> 8 debug bits); a release build answers those flags with an error.  The A/B kernels of rounds 3-4 that
 * were measured slower (row-stationary bf16, three-term fp32 split, four-workgroup ring, deferred accumulate, eight-wave
 * workgroups) were removed in round 5, the register-accumulator kernel over the gather table (k_conv_rb, 0.73-0.91x) in
 * round 6; their tables under profiles/ are the record.                                  */
int aabr_build_flags(void);
/* number of int32 words of the `meta` block written by the geometry builders */
#define AABR_META_WORDS 16
/* meta[0] = number of active sites, meta[1] = max points per site (input layer only; brick levels: number of bricks),
 * meta[2] = error flag (non-zero: coordinate out of range), meta[3] = total of 2nd scan lane,
 * meta[4], meta[5] = internal (chunk ticket, redo flag of the packed input-layer forms),
 * meta[8..11] (input layer) = largest x, y, z and batch index over the valid points, -1 when there is none: the extent
 * a brick grid's directory is sized by */

/* ---- input pipeline ---------------------------------------------------------------------------
 * Device-side form of the dataset's host quantisation (data3d/suncg_utils/suncg_dataset.py:126-188,
 * test-time path: no augmentation): a = xyz*scale - min(xyz)*scale; keep 0 <= a < full_scale;
 * locs = trunc(a) (int64 [n,4], 4th column = batch_index); feats_xyz (optional, float32 rows of
 * stride feat_stride) receives a/scale.  xyz / xyz_min are float32 or float64 device arrays
 * ([n,3] / [3]); full_scale_dev int32[3] on the device.  Points outside the range are not
 * compacted away: they get the coordinate sentinel (-1,-1,-1), which aabr_input_layer_sites skips
 * (the reference drops them on the host before the input layer, suncg_dataset.py:183-185).      */
int aabr_quantize_points(const void *xyz, int is_double, int64_t n, double scale, const void *xyz_min,
                         const int32_t *full_scale_dev, int64_t batch_index, int64_t *locs,
                         float *feats_xyz, int feat_stride, void *stream);
/* The same quantisation for a PADDED batch -- the [B, L, 3] / [B, L, C] pair BLInputLayer consumes (ioLayers.py:92-136) --
 * for all scenes at once; replaces the per-scene host loop of the dataset + trainMerge collate (suncg_dataset.py:126-188,
 * data3d/data.py:25-37) and, on this side, one minimum, one aabr_quantize_points launch and one feature copy per scene.
 *   xyz_host / extra_host  HOST arrays of `scenes` device pointers: [n_b, 3] float32 or float64 (is_double, one type for
 *                          the batch) and [n_b, extra_planes] float32 (extra_host may be NULL when extra_planes == 0)
 *   n_host                 host int64 [scenes], every n_b <= L
 *   coords int64 [scenes, L, 3], feats float32 [scenes, L, 3 + extra_planes]: every element is written --
 *     row l < n_b: the scene's quantised point ((-1,-1,-1) outside full_scale; features a / scale, then the extra row);
 *     rows n_b .. L-1: -1 coordinates, zero features.
 *   min_keys  uint64 [3 * scenes] device scratch (the per-scene minimum, as order-preserving keys).
 * The pointers and sizes of up to 32 scenes travel by value in the kernel arguments: one fill + two launches (minimum,
 * quantise + feature copy) for scenes <= 32, two more launches per further 32.  No host read.  Inputs are finite.      */
int aabr_quantize_scenes_bl(const void *const *xyz_host, const void *const *extra_host, const int64_t *n_host,
                            int scenes, int is_double, int extra_planes, double scale, const int32_t *full_scale_host,
                            int64_t L, int64_t *coords, float *feats, uint64_t *min_keys, void *stream);

/* ---- hash grid ---------------------------------------------------------------------------
 * A grid is an open-addressing table of cap 16-byte entries {uint64 key (packed b,x,y,z), uint32 first, int32 val
 * (row of the site)}, handed over through the `keys` parameters (16-byte aligned).  cap must be a power of two
 * >= 2 * (number of inserted keys).  Probing is linear inside the key's home block of 4096 slots (csrc/common.h
 * grid_next): a probe chain stays inside one 64 KiB window and the LDS-binned voxel scatter can build a block per
 * workgroup.
 * Replaces SparseGrid / SparseGridMap (SCN/Metadata/Metadata.h:24-33).                       */

/* Voxel scatter, geometry half -- replaces Metadata<3>::inputLayer -> inputLayerRules
 * (SCN/Metadata/Metadata.cpp:405-417, IOLayersRules.h:18-125), modes 1..4.  One fill + two kernels
 * (csrc/voxel_scatter.hip): hash insert + first-point atomicMin; then ONE pass over the points that numbers the
 * voxels in first-seen order (chunk scan + decoupled look-back) and links every further point of a voxel into
 * the site's chain.
 *   coords       int64 [n, ncols] (ncols 3 or 4; 4th column = batch index)   (API layout)
 *   keys         the hash grid: cap entries of 16 bytes {uint64 key, uint32 first, int32 val}, 16-byte aligned,
 *                contents overwritten (interleaved so that the insert's CAS, its first-seen minimum and every
 *                later probe of a slot touch one 64-byte sector); followed directly by `meta` the two are cleared
 *                with a single fill
 *   slot         int32 [n]   scratch: hash slot of every point
 *   point_site   int32 [n]   out: output row of every input row (-1: dropped)
 *   site_coords  int32 [n,4] out: first V rows valid, first-seen order
 *   first_pt     int32 [n]   out: first (lowest-index) point of each site
 *   cnt_extra    int32 [n]   out: points per site minus one
 *   head, nxt    int32 [n]   out: chain of the site's further points (head[site] -> nxt[point] -> ... -> -1)
 *   status       int32 [aabr_input_layer_status_words(n)] scratch (8-byte aligned)
 *   meta         int32 [AABR_META_WORDS] out (device): V, (maxActive: written by aabr_input_layer_forward), error */
int64_t aabr_input_layer_status_words(int64_t n);
int aabr_input_layer_sites(const int64_t *coords, int64_t n, int ncols, uint64_t *keys, int64_t cap,
                           int32_t *slot, int32_t *point_site, int32_t *site_coords, int32_t *first_pt,
                           int32_t *cnt_extra, int32_t *head, int32_t *nxt, int32_t *status, int32_t *meta,
                           void *stream);
/* The same result (site list, first-seen numbering, chains, finished hash grid) by the two forms BASELINE.json's
 * north_star asks about, for inputs whose (batch, x, y, z, point index) fit ONE 64-bit word -- field widths from the
 * layer's spatial size (IOLayersRules.h:18-125 receives it as `spatialSize`) and n; aabr_input_layer_pack_bits returns
 * the bits left for the batch index (0: does not fit, use aabr_input_layer_sites):
 *   variant 1  one device atomic per point (CAS of the word into an 8-byte side table, atomicMin only for the
 *              smaller of two points of one voxel) instead of two;
 *   variant 2  LDS-staged hash binning with coalesced HBM writes and no device atomics on the table: the words are
 *              partitioned by hash block (4096 slots), every block's table is built in LDS by one workgroup and its
 *              4096 finished 16-byte entries are written with coalesced stores (no fill of the grid).
 * words: cap 8-byte words of scratch (side table / record regions); cursor: cap/4096 int32 (variant 2; 4096 <= cap
 * <= 2^24).  When a point does not fit the word (coordinate >= spatial size, batch index beyond the bits left) or a
 * block overflows its record region, meta[5] comes back 0 (else -1) and the caller must run aabr_input_layer_sites
 * on the same buffers instead; the other outputs are then unspecified.  n > 0.                                */
int aabr_input_layer_pack_bits(int64_t n, const int32_t *spatial_host);
int aabr_input_layer_sites_packed(const int64_t *coords, int64_t n, int ncols, const int32_t *spatial_host,
                                  int variant, uint64_t *keys, int64_t cap, uint64_t *words, int32_t *cursor,
                                  int32_t *slot, int32_t *point_site, int32_t *site_coords, int32_t *first_pt,
                                  int32_t *cnt_extra, int32_t *head, int32_t *nxt, int32_t *status, int32_t *meta,
                                  void *stream);
/* aabr_input_layer_sites for the BATCHED layout -- replaces Metadata<3>::blLayer -> blRules (SCN/Metadata/Metadata.cpp:419-428,
 * IOLayersRules.h:127-297; pybind.cpp:171-175 BLInputLayer_updateOutput, SCN/CPU/IOLayers.cpp:138-230).  coords is int64
 * [B, L, 3], read where it lies: point i is the flat row i = b * L + l and its batch index is i / L -- no [B L, 4] copy.
 *   A row is EMPTY if and only if x < 0, whatever y and z hold (`if (p[0] >= 0)`, IOLayersRules.h:188,203,256): it is
 *   skipped silently, point_site = -1.  (The flat form's sentinel is x == y == z == -1.)
 *   A row with x >= 0 and a negative y or z, or any coordinate above 65534, sets the error word meta[2].
 *   Sites are numbered by first appearance in ascending flat row: sample-major (all sites of sample 0, then sample 1, ...),
 *   first-seen inside a sample -- blRules' `SGs[I].ctr` + `nAct++`; the same coordinate in two samples is two sites.
 * Same kernels (the generic hash form), same launches, same outputs and buffer sizes as aabr_input_layer_sites with
 * n = B * L; the packed and LDS-binned inserts are not offered for this layout.  0 <= B <= 65535, B * L < 2^31;
 * B * L == 0 launches nothing.                                                                                          */
int aabr_bl_input_layer_sites(const int64_t *coords, int64_t B, int64_t L, uint64_t *keys, int64_t cap,
                              int32_t *slot, int32_t *point_site, int32_t *site_coords, int32_t *first_pt,
                              int32_t *cnt_extra, int32_t *head, int32_t *nxt, int32_t *status, int32_t *meta,
                              void *stream);

/* Voxel scatter, feature half -- replaces InputLayer_ForwardPass / InputLayer_fp_
 * (SCN/CPU/IOLayers.cpp:11-29, SCN/CUDA/IOLayers.cu:14-41).  mode: 1 keep-first-listed,
 * 2 keep-last-listed, 3 sum, 4 mean (exactly the reference's mode table, ioLayers.py:33-38).
 * Also writes last_pt [V] (highest-index point of each site; may be NULL) and meta[1] = maxActive. */
int aabr_input_layer_forward(const float *in_feats, float *out_feats, int64_t V, int planes,
                             const int32_t *first_pt, const int32_t *cnt_extra, const int32_t *head,
                             const int32_t *nxt, int32_t *last_pt, int mode, int32_t *meta, void *stream);
/* replaces InputLayer_BackwardPass / InputLayer_bp_ (CPU/IOLayers.cpp:30-47, IOLayers.cu:43-70) */
int aabr_input_layer_backward(float *d_in_feats, const float *d_out_feats, int64_t n, int planes,
                              const int32_t *point_site, const int32_t *first_pt, const int32_t *last_pt,
                              const int32_t *cnt_extra, int mode, void *stream);

/* Reference-format input rule table rules[1] (IOLayersRules.h:112-124): int32 [V, 1+maxActive]. */
int aabr_input_layer_rule_table(const int32_t *first_pt, const int32_t *last_pt, const int32_t *cnt_extra,
                                const int32_t *head, const int32_t *nxt, int64_t V, int max_active, int mode,
                                int32_t *rules, void *stream);

/* Submanifold rule table -- replaces Metadata<3>::getSubmanifoldRuleBook ->
 * SubmanifoldConvolution_SgToRules (Metadata.cpp:429-443, SubmanifoldConvolutionRules.h:11-45).
 * table[k*V + v] = row of the site at coords[v] + offset_k (offset enumeration of
 * RectangularRegion::offset, RectangularRegions.h:30-38: z fastest), or -1.
 * counts (int32 [vol * ceil(V/256)], optional) receives per-offset, per-256-row-block rule
 * counts (sum over the second index = rules at that offset).                                 */
int aabr_submanifold_table(const int32_t *site_coords, int64_t V, const uint64_t *keys,
                           int64_t cap, const int32_t *filter_size_host,
                           int32_t *table, int32_t *counts, void *stream);

/* Per-sample row offsets of a batch-contiguous site list -- replaces SparseGrid::ctr (Metadata.h:24-33; read by
 * Metadata::getSpatialLocations, Metadata.cpp:147-168, and by the anchor generator's per-example index scopes,
 * anchor_generator_sparse3d.py:137-147).  out int32 [max_samples + 2]: out[0] = V (read from meta[0] on the device,
 * clipped to V_max), out[1 + b] = first row with batch index >= b for b = 0 .. max_samples.                    */
int aabr_sample_offsets(const int32_t *site_coords, const int32_t *meta, int64_t V_max, int max_samples,
                        int32_t *out, void *stream);

/* ---- brick grids (extension; csrc/brick.hip, csrc/geom.h) -------------------------------------------------------------
 * A level of the scene stored by WHERE its sites are instead of in a hash table -- what replaces the reference's
 * per-sample google::dense_hash_map (Metadata.h:24-34) when Metadata_3 is created with site_order="brick":
 *   dir    [nb * sbx * sby * sbz] 16-byte entries {uint64 word, uint32 prefix, pad}: one entry per super-brick (16^3 voxels)
 *          of the level's extent, one bit per brick (4^3 voxels), prefix = occupied bricks in front of the word;
 *   bricks [NB] 16-byte entries {uint64 cell mask, int32 base, pad} in directory order, base = sites in front of the brick;
 *   row of the site at (b, x, y, z) = base + popcount(mask below cell (x&3)<<4 | (y&3)<<2 | (z&3)).
 * dims_host = {sbx, sby, sbz, nb}.  Sites are numbered brick by brick, cell by cell: spatial neighbours are neighbours
 * in memory, a lookup is two dependent 16-byte loads (no hashing), and the row order inside a sample is a permutation
 * of the reference's first-seen order (parity modulo a per-sample permutation).
 *
 * aabr_brick_build: the level that holds, for every input site u < min(vin_bound, *vin_count_dev) (vin_count_dev may
 * be NULL) and every cell of its output region under (size, stride, out_spatial) (OutputRegionCalculator,
 * RectangularRegions.h:109-119; size = stride = 1: the level of the input sites themselves; size == stride up to 65536:
 * the composition of non-overlapping levels as in aabr_convolution_sites), one site -- what
 * Convolution_InputSgToRulesAndOutputSg creates (ConvolutionRules.h:11-34).  Writes dir, bricks, bcoord [NB] int32x4
 * brick coordinates, out_coords [V] int32x4 (x, y, z, batch) in row order and meta (meta[0] = V, meta[1] = NB, meta[2] != 0:
 * a site outside the extent `dims` covers, or more than nb_cap bricks / v_cap sites).  Nothing is read back: a chain of
 * levels is enqueued back to back with device-side counts.  scratch: aabr_brick_scratch_words(dir words, nb_cap) int32.
 * flags bit 0: the caller has zeroed dir, bricks, meta and scratch (a pyramid's levels share ONE fill).  A one-workgroup
 * form for the coarse levels (every phase in a single launch) was built and measured slower than the eight small launches it
 * replaced (returning atomics in a serial loop: 930 vs 615 us for the 12 strided grids of the bench batch) and removed.  */
int64_t aabr_brick_scratch_words(int64_t dir_words, int64_t nb_cap);
int aabr_brick_build(const int32_t *in_coords, int64_t vin_bound, const int32_t *vin_count_dev, const int32_t *size_host,
                     const int32_t *stride_host, const int32_t *out_spatial_host, const int32_t *dims_host, void *dir,
                     void *bricks, int64_t nb_cap, int32_t *bcoord, int32_t *out_coords, int64_t v_cap, int32_t *meta,
                     int32_t *scratch, int flags, void *stream);
/* aabr_brick_full_build: the DILATING level build -- the level a FullConvolution / TransposeConvolution writes to, brick-major:
 * one site at u * stride + q for every input site u and every filter offset q in [0, size) (the serial host loop of
 * FullConvolution_InputSgToRulesAndOutputSg over a hash map, FullConvolutionRules.h:11-33, with InputRegionCalculator,
 * RectangularRegions.h:95-105).  Arguments, outputs, scratch and flags as aabr_brick_build; out_spatial = the NEW level's
 * spatial size (in - 1) * stride + size (<= 65535 per axis), a candidate outside it sets meta[2]; per-axis limits of
 * aabr_brick_build; vin_bound * prod(size) must stay below 2^31.  Each parent site marks its prod(size) cells, then the same
 * scans and expansion: no hash table, integer atomics only (the bit-setting OR), rows a function of the site set alone.   */
int aabr_brick_full_build(const int32_t *in_coords, int64_t vin_bound, const int32_t *vin_count_dev,
                          const int32_t *size_host, const int32_t *stride_host, const int32_t *out_spatial_host,
                          const int32_t *dims_host, void *dir, void *bricks, int64_t nb_cap, int32_t *bcoord,
                          int32_t *out_coords, int64_t v_cap, int32_t *meta, int32_t *scratch, int flags, void *stream);
/* Input level: the voxel scatter numbers its sites in first-seen order (IOLayersRules.h:86-91); old_coords [V] are those
 * sites, (dir, bricks) the brick level built from them.  new_of_old[r] / old_of_new[i] = the permutation; first_pt /
 * cnt_extra / head re-indexed by the new rows; point_site2[p] = new row of point p's site.                           */
int aabr_brick_renumber(const int32_t *old_coords, int64_t V, const int32_t *dims_host, const void *dir, const void *bricks,
                        int32_t *new_of_old, int32_t *old_of_new, const int32_t *first_pt, const int32_t *cnt_extra,
                        const int32_t *head, int32_t *first_pt2, int32_t *cnt_extra2, int32_t *head2,
                        const int32_t *point_site, int64_t n, int32_t *point_site2, int32_t *meta, void *stream);
/* Voxel scatter straight into a brick grid -- InputLayer (Metadata::inputLayer -> inputLayerRules, Metadata.cpp:405-417,
 * IOLayersRules.h:18-125) without a hash table and without first-seen numbers: the POINTS are the items of the input
 * level's aabr_brick_build (size = stride = 1), a voxel's row follows from where it lies.
 *   aabr_points_prepare: coords int64 [n, ncols] -> pc int32 [n,4] (x, y, z, batch; x = -1: a point the layer skips),
 *     meta (AABR_META_WORDS, starts at all ones): meta[2] == 0: a coordinate outside [0, 65534]; meta[8..11] = largest
 *     x, y, z, batch index of the valid points (-1: none) -- the extent the directory is sized by.  first_pt / cnt_extra /
 *     head (each n words; all three or none, may be NULL): set to their starting values (-1, 0, -1) in the same pass, so
 *     aabr_points_sites (flags bit 0) need not fill them.
 *   aabr_points_sites (after aabr_brick_build(pc, n, ..)): point_site[i] = row of point i's voxel (-1: skipped),
 *     first_pt[row] = lowest point index of the voxel, cnt_extra[row] = its further points, head / nxt = their chain --
 *     the arrays aabr_input_layer_forward / _backward / _rule_table read; sized n (rows < V are meaningful).
 *     flags bit 0: first_pt / cnt_extra / head already hold their starting values (aabr_points_prepare wrote them).   */
int aabr_points_prepare(const int64_t *coords, int64_t n, int ncols, int32_t *pc, int32_t *meta, int32_t *first_pt,
                        int32_t *cnt_extra, int32_t *head, void *stream);
int aabr_points_sites(const int32_t *pc, int64_t n, const int32_t *dims_host, const void *dir, const void *bricks,
                      int32_t *point_site, int32_t *first_pt, int32_t *cnt_extra, int32_t *head, int32_t *nxt,
                      int32_t *meta, int flags, void *stream);
/* aabr_points_prepare for the batched layout (blRules, IOLayersRules.h:127-297; see aabr_bl_input_layer_sites for the
 * empty-row and error rules): coords int64 [B, L, 3] read in place -> pc int32 [B L, 4] with pc[i].w = i / L.  The same
 * kernel body; aabr_brick_build / aabr_points_sites follow as for the flat list.  meta[11] is the largest NON-EMPTY
 * sample; the caller that wants B samples (trailing empty ones included) sizes the directory by B itself.          */
int aabr_bl_points_prepare(const int64_t *coords, int64_t B, int64_t L, int32_t *pc, int32_t *meta, int32_t *first_pt,
                           int32_t *cnt_extra, int32_t *head, void *stream);
/* aabr_submanifold_table / aabr_convolution_tables2 over brick levels: same tables, same block counts
 * (Metadata.cpp:429-443,484-510; SubmanifoldConvolutionRules.h:26-45; ConvolutionRules.h:11-34).                       */
int aabr_brick_submanifold_table(const int32_t *site_coords, int64_t V, const int32_t *dims_host, const void *dir,
                                 const void *bricks, const int32_t *filter_size_host, int32_t *table, int32_t *counts,
                                 void *stream);
int aabr_brick_convolution_tables(const int32_t *in_coords, int64_t V_in, const int32_t *in_dims_host, const void *in_dir,
                                  const void *in_bricks, const int32_t *out_coords, int64_t V_out,
                                  const int32_t *out_dims_host, const void *out_dir, const void *out_bricks,
                                  const int32_t *size_host, const int32_t *stride_host, const int32_t *out_spatial_host,
                                  int32_t *table_out, int32_t *table_in, int32_t *counts, int32_t *counts_in, void *stream);

/* Strided convolution geometry -- replaces Metadata<3>::getRuleBook ->
 * Convolution_InputSgToRulesAndOutputSg (Metadata.cpp:484-510, ConvolutionRules.h:11-34,
 * RectangularRegions.h:95-119).  Creates the output grid (sites numbered in first-seen order
 * over input rows ascending, then output-region order) and reports V_out in meta[0].
 *   out_keys: out_cap 16-byte grid entries as in aabr_input_layer_sites, out_cap a power of two >= 1.5 E;
 *   scratch int32 [E + 4*ceil(E/256) + 16], E = V_in * max_out_per_in,
 *   max_out_per_in = prod(ceil(size/stride)); out_site_coords int32 [E,4].
 * size, stride <= 64 per axis; for size == stride (one output site per input site) up to 65536, so that a chain of
 * non-overlapping levels can be built from its FIRST grid in one step each (size = stride = product of the chain's
 * strides): the site set and its first-seen order are those of the level-by-level construction.          */
int aabr_convolution_sites(const int32_t *in_coords, int64_t V_in, const int32_t *size_host,
                           const int32_t *stride_host, const int32_t *out_spatial_host,
                           uint64_t *out_keys, int64_t out_cap,
                           int32_t *scratch, int32_t *out_site_coords, int32_t *meta,
                           void *stream);
/* FullConvolution / TransposeConvolution geometry -- replaces Metadata<3>::getFullConvolutionRuleBook ->
 * FullConvolution_InputSgToRulesAndOutputSg (Metadata.cpp:511-531, FullConvolutionRules.h:11-33, RectangularRegions.h:95-105):
 * the level that GROWS.  Creates the grid that holds one site at u * stride + q for every input site u and every filter
 * offset q in [0, size); sites are numbered in first-seen order over input rows ascending, then offsets with z fastest
 * (what an insertion-ordered map gives the reference's loop; samples stay contiguous and in batch order); V_out in meta[0].
 * Arguments as aabr_convolution_sites with E = V_in * prod(size) candidates (E < 2^31): out_cap a power of two >= 1.5 E,
 * scratch int32 [E + 4*ceil(E/256) + 16], out_site_coords int32 [E,4]; out_spatial = the new level's spatial size
 * (in - 1) * stride + size, <= 65535 per axis -- a candidate outside it is left out and sets meta[2].  Per-axis limits of
 * aabr_convolution_sites.  V_in = 0: the grid is cleared, meta[0] = 0, no launch.  The rule tables of the layer are
 * aabr_convolution_tables2 with the new level as the convolution's INPUT side and the layer's input level as its output
 * side: table_out is complete by construction, table_in is what the forward pass gathers through.                       */
int aabr_full_convolution_sites(const int32_t *in_coords, int64_t V_in, const int32_t *size_host,
                                const int32_t *stride_host, const int32_t *out_spatial_host, uint64_t *out_keys,
                                int64_t out_cap, int32_t *scratch, int32_t *out_site_coords, int32_t *meta, void *stream);
/* counts (optional): int32 [vol * ceil(V_out/256)] per-block rule counts, as above.
 * table_out[k*V_out + o] = input row at offset k of output o's window (or -1);
 * table_in [k*V_in  + u] = output row whose window holds input u at offset k (or -1).
 * A filter volume above 65535 is refused (AABR_EINVAL), as by aabr_submanifold_table.       */
int aabr_convolution_tables(const int32_t *in_coords, int64_t V_in, const uint64_t *in_keys,
                            int64_t in_cap,
                            const int32_t *out_coords, int64_t V_out, const uint64_t *out_keys,
                            int64_t out_cap, const int32_t *size_host,
                            const int32_t *stride_host, const int32_t *out_spatial_host,
                            int32_t *table_out, int32_t *table_in, int32_t *counts,
                            void *stream);
/* the same with the per-block rule counts of table_in as well (counts_in int32 [vol * ceil(V_in/256)], may be
 * NULL): what the weight-gradient pass of a transposed convolution sizes its chunks with.               */
int aabr_convolution_tables2(const int32_t *in_coords, int64_t V_in, const uint64_t *in_keys,
                            int64_t in_cap,
                            const int32_t *out_coords, int64_t V_out, const uint64_t *out_keys,
                            int64_t out_cap, const int32_t *size_host,
                            const int32_t *stride_host, const int32_t *out_spatial_host,
                            int32_t *table_out, int32_t *table_in, int32_t *counts,
                             int32_t *counts_in, void *stream);

/* Reference-format rule book from a gather table: for offset k the (in,out) pairs in
 * ascending `out` order -- the layout of RuleBook = vector<vector<Int>> (Metadata.h:34).
 * rules int32 [vol][V][2] (first counts[k] pairs of each slab valid); in_col selects which
 * column receives the table entry (0: table entry = input row; 1: swapped / deconvolution).  */
int aabr_table_to_rulebook(const int32_t *table, int64_t V, int vol, int32_t *rules,
                           int32_t *counts, void *stream);

/* Metadata<3>::getSpatialLocations (Metadata.cpp:147-168): int32 [V,4] -> int64 [V,4]. */
int aabr_spatial_locations(const int32_t *site_coords, int64_t V, int64_t *locations,
                           void *stream);

/* ---- compiled rule books -------------------------------------------------------------------
 * A gather table is compiled once per rule book (and reused by every layer at that scale, forward
 * and backward) into the two streaming layouts the MFMA kernels read:
 *  (1) tile blocks: for each tile of 64 output rows, blocks of 16 (partner row, local row) pairs
 *      that share one filter offset -- input of aabr_conv_forward;
 *  (2) offset pairs: for each offset the (partner row, row) pairs in ascending row order -- the
 *      reference's RuleBook layout (Metadata.h:34) -- input of aabr_conv_backward_weight.
 * block_counts is the `counts` output of the table builder.  Limits: V < 2^25.                   */
int64_t aabr_tile_blocks_words(int64_t V, int vol);   /* int32 words of `blocks` */
int aabr_build_tile_blocks(const int32_t *table, int64_t V, int vol, int32_t *blocks, void *stream);
int64_t aabr_offset_pairs_words(int64_t V, int vol);  /* int32 words of `pairs` */
int aabr_build_offset_pairs(const int32_t *table, const int32_t *block_counts, int64_t V, int vol,
                            int32_t *pairs, void *stream);

/* Wide-layer forms of the same contraction (csrc/conv_wide.hip): 128-row output tiles whose blocks
 * share one set of weights per filter offset (registers / LDS) instead of streaming 32 KiB of packed weights per
 * 16-pair block.  Replaces the same reference loops as aabr_conv_forward (SCN/CPU/Convolution.cpp:45-185,
 * SCN/CPU/Deconvolution.cpp:7-77; the CUDA twin it stands in for is dConvolution_KMxKN_forwardA/B,
 * SCN/CUDA/Convolution.cu:57-203).
 *   aabr_conv_wide_tile_rows: 0 = use aabr_conv_forward; 128 = rows per tile of the block stream that
 *     aabr_conv_forward_wide wants for this shape (supported AND expected to beat the 64-row-tile kernels);
 *   aabr_wide_blocks_words / aabr_build_wide_blocks: gather table [vol][V] -> per-tile per-offset blocks of 16
 *     (partner row, local row) pairs (vol <= 63);
 *   aabr_conv_pack_weights: W [vol][nIn][nOut] (transpose: W[k]^T) -> packed MFMA A-operand layout;
 *   aabr_conv_forward_wide: n_in % 32 == 0, n_out % 64 == 0; `wpack` must already hold the packed weights of
 *     this orientation; flags bit1: mirrored offsets (submanifold input-gradient through the forward table). */
int aabr_conv_wide_tile_rows(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol);
int64_t aabr_wide_blocks_words(int64_t V, int vol, int tile_rows);
int aabr_build_wide_blocks(const int32_t *table, int64_t V, int vol, int tile_rows, int32_t *blocks, void *stream);
int aabr_conv_pack_weights(const float *W, int vol, int n_in, int n_out, int transpose, float *wpack, void *stream);
int aabr_conv_forward_wide(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                           int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                           int flags, const float *wpack, void *stream);
/* the same with out = conv + residual ([V_out, n_out] fp32, may be NULL): the residual / lateral add that follows
 * the convolution in the reference's graph (AddTable, tables.py:27-41; add_feature_planes, utils.py:38-44) folded
 * into the write-out; a + b is commutative bit for bit, so the result equals the separate add's.           */
int aabr_conv_forward_wide_res(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                               int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                               int flags, const float *wpack, const float *residual, void *stream);
/* the same, and the write-out also forms the TRAINING STATISTICS of the BatchNormalization that reads this output
 * (replaces the statistics loop of SCN/CPU/BatchNormalization.cpp:20-32 / the first reduction of
 * SCN/CUDA/BatchNormalization.cu:14-72 -- one read pass over the feature matrix less): per output tile one
 * [2][n_out] pair of fp64 column sums (sum x, sum x^2) of exactly the values stored (after bias / residual, after the
 * bf16 rounding), at stats[tile * 2 * n_out ...]; aabr_conv_wide_stats_doubles() doubles, tile_rows >= 64.  Hand
 * them to aabr_bn_forward_parts with nparts = ceil(V_out / tile_rows): it combines them in tile order, so the
 * result is reproducible bit for bit.  stats == NULL: plain aabr_conv_forward_wide_res.                        */
int64_t aabr_conv_wide_stats_doubles(int64_t V_out, int tile_rows, int n_out);
int aabr_conv_forward_wide_stats(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                                 int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                                 int flags, const float *wpack, const float *residual, double *stats, void *stream);
int aabr_conv_forward_wide_bf16_stats(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats,
                                      int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                      const float *bias, int flags, const uint16_t *wpack, double *stats, void *stream);
/* Single-rule form (csrc/conv_single.hip, fp32 storage): the same contraction for rule books in which EVERY OUTPUT ROW
 * HAS EXACTLY ONE RULE -- out[o] = in[i(o)] @ Wl[k(o)] (+ bias, + residual) -- as in the reference's Deconvolution with
 * filter == stride (SCN/CPU/Deconvolution.cpp:7-77) and its 1x1x1 SubmanifoldConvolution, forward and input gradient.
 * THE CALLER GUARANTEES that property: the library cannot see it; a row named by several rules would hold one of their
 * terms, a row named by none is not written.  Reads the offset pairs of aabr_build_offset_pairs (built over the
 * launch's gather table [vol][V_out]) instead of tile blocks; `wpack` as aabr_conv_forward_wide (the orientation of the
 * launch: the input-gradient form hands over the transposed pack and the same pairs); flags bit1: mirrored offsets.
 * n_in % 32 == 0, n_in <= 128, n_out % 64 == 0.  No fp32 output tile, no weight reload per tile: one MFMA chain per
 * output element in the K order of aabr_conv_forward_wide, then + bias, + residual -- the result equals
 * aabr_conv_forward_wide_res's bit for bit.
 *   aabr_conv_single_chunk: pairs per chunk (256 / 1024) when such a launch should take this form, else 0 (bf16 storage,
 *     statistics wanted in the write-out, an unsupported shape, too few rows, knob CONV_SINGLE = 0);
 *   aabr_conv_single_refusal: why it returned 0 ("" when it did not).                                              */
int aabr_conv_single_chunk(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, int bf16, int has_stats);
const char *aabr_conv_single_refusal(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, int bf16,
                                     int has_stats);
int aabr_conv_forward_single(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                             int64_t V_out, const int32_t *pairs, int vol, const float *bias, int flags,
                             const float *wpack, const float *residual, void *stream);
/* The single-rule form as an INPUT-GRADIENT launch whose output is the d_out of a BatchNormalization(+leaky ReLU) -- the
 * input gradient of a Convolution with filter == stride, every fine row having one parent: the write-out also forms that
 * BatchNorm's backward statistics, term for term those of aabr_conv_forward_wide_bwd_stats below, whose BatchNorm
 * arguments it takes in the same order; `out_feats` equals aabr_conv_forward_single's bit for bit.  `stats` receives
 * aabr_conv_single_bwd_stats_parts(V_out, vol, chunk) parts of [2][n_out] fp64 sums, one per chunk of the pair list
 * (chunks without pairs write zeros), to be summed in part order (aabr_bn_backward_parts); no atomics.  fp32 storage.
 *   aabr_conv_single_bwd_stats_chunk: pairs per chunk when such a launch should take this form, else 0 (the conditions of
 *     aabr_conv_single_chunk without the statistics one; knob SINGLE_BWD_STATS = 0).  `has_stats` of the two queries
 *     above means statistics this plain form does not deliver: they keep refusing it;
 *   aabr_conv_single_bwd_stats_refusal: why it returned 0 ("" when it did not).                                    */
int aabr_conv_single_bwd_stats_chunk(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, int bf16);
const char *aabr_conv_single_bwd_stats_refusal(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, int bf16);
int64_t aabr_conv_single_bwd_stats_parts(int64_t V_out, int vol, int chunk_pairs);
int aabr_conv_forward_single_bwd_stats(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                                       int64_t V_out, const int32_t *pairs, int vol, const float *bias, int flags,
                                       const float *wpack, const float *residual, double *stats, const float *bn_in,
                                       const float *save_mean, const float *save_invstd, const float *bn_weight,
                                       const float *bn_bias, float leakiness, void *stream);
/* Input-gradient form of the same launch (flags = transposed | mirrored, as aabr_conv_forward_wide): its output is the
 * d_out of the BatchNormalization(+leaky ReLU) whose result the convolution consumed; the write-out forms THAT
 * BatchNorm's backward statistics (replaces the first loop of BatchNormalization_BackwardPass,
 * SCN/CPU/BatchNormalization.cpp:66-84): per tile [2][n_out] fp64 sums of d and (x - mean) * d, d = d_out masked by the
 * sign of the forward activation recomputed from the BatchNorm input `bn_in` (leakiness >= 0).  fp32 storage.      */
int aabr_conv_forward_wide_bwd_stats(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                                     int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                                     int flags, const float *wpack, const float *residual, double *stats,
                                     const float *bn_in, const float *save_mean, const float *save_invstd,
                                     const float *bn_weight, const float *bn_bias, float leakiness, void *stream);
/* ... and the BatchNorm backward that takes them (nparts = ceil(rows / tile_rows)); everything else as
 * aabr_bn_backward_add (d_in_add may be NULL).                                                                   */
int aabr_bn_backward_parts(const float *in, float *d_in, const float *out, const float *d_out, int64_t rows, int planes,
                           const float *save_mean, const float *save_invstd, const float *weight, const float *bias,
                           float *d_weight, float *d_bias, float leakiness, const double *parts, int nparts,
                           float *scratch, const float *d_in_add, void *stream);
/* bf16 storage of the two: the sign comes from the BatchNorm's STORED output `bn_out` (as aabr_bn_backward_bf16 reads
 * it), x and d are the stored (rounded) values, sums in fp64 -- the same terms k_bn_partials forms.               */
int aabr_conv_forward_wide_bf16_bwd_stats(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats,
                                          int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                          const float *bias, int flags, const uint16_t *wpack, double *stats,
                                          const uint16_t *bn_in, const uint16_t *bn_out, const float *save_mean,
                                          float leakiness, void *stream);
/* The general bf16-storage launch of the compiled pass: aabr_conv_forward_wide_bf16 with an optional `residual` (bf16
 * [V_out, n_out]: out = bf16(bf16(conv + bias) + residual) -- the residual / lateral add, or the gradient sum of a tensor
 * with a second consumer, folded into the write-out, bit for bit what the separate bf16 add stores), optional `stats`
 * of the stored values (as aabr_conv_forward_wide_bf16_stats; bn_in NULL) or, with bn_in / bn_out / save_mean /
 * leakiness, the backward statistics of aabr_conv_forward_wide_bf16_bwd_stats.                                        */
int aabr_conv_forward_wide_bf16_res(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats, int n_out,
                                    int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                                    int flags, const uint16_t *wpack, const uint16_t *residual, double *stats,
                                    const uint16_t *bn_in, const uint16_t *bn_out, const float *save_mean, float leakiness,
                                    void *stream);
int aabr_bn_backward_parts_bf16(const uint16_t *in, uint16_t *d_in, const uint16_t *out, const uint16_t *d_out,
                                int64_t rows, int planes, const float *save_mean, const float *save_invstd,
                                const float *weight, const float *bias, float *d_weight, float *d_bias, float leakiness,
                                const double *parts, int nparts, float *scratch, void *stream);
/* BatchNormalization forward in training mode with the statistics' partial sums given (layout above; any producer
 * that writes [nparts][2][planes] fp64 sums of x and x^2 will do): everything else as aabr_bn_forward[_bf16].   */
int aabr_bn_forward_parts(const float *in, float *out, int64_t rows, int planes, float *save_mean,
                          float *save_invstd, float *running_mean, float *running_var, const float *weight,
                          const float *bias, float eps, float momentum, float leakiness, const double *parts,
                          int nparts, float *scratch, void *stream);
int aabr_bn_forward_parts_bf16(const uint16_t *in, uint16_t *out, int64_t rows, int planes, float *save_mean,
                               float *save_invstd, float *running_mean, float *running_var, const float *weight,
                               const float *bias, float eps, float momentum, float leakiness, const double *parts,
                               int nparts, float *scratch, void *stream);

/* Name of the kernel instance (template arguments included) the last aabr_conv_forward[_bf16] /
 * aabr_conv_backward_weight[_bf16] call on this thread dispatched -- measurement provenance only.   */
const char *aabr_conv_last_variant(void);

/* ---- sparse convolution (fp32 features, fp32 MFMA) ----------------------------------------
 * out[o] = bias + sum_k in[table[k][o]] @ W[wk(k)]      (rows with table == -1 contribute 0)
 * Replaces {Submanifold,}Convolution_updateOutput / Deconvolution_updateOutput
 * (SCN/sparseconvnet_cuda.cpp:281-310; CPU/Convolution.cpp:45-79,117-149;
 *  CPU/Deconvolution.cpp:7-41; CUDA/Convolution.cu:57-233,444-521,618-642).
 *   rows_in  number of rows of `in_feats` (bounds the gather; V_out for submanifold layers)
 *   blocks   tile blocks compiled from the gather table whose entries index `in_feats`
 *   W        float32 [vol, nIn, nOut]  (the reference's [vol, groups=1, nIn, nOut])
 *   flags    bit0: use W[k]^T (input-gradient pass: `in` has nOut planes, `out` nIn planes,
 *            CPU/Convolution.cpp:108-112); bit1: weight index vol-1-k (submanifold
 *            input-gradient through the forward table); bit2: `wpack` already holds the packed
 *            weights for this (W, bit0) pair (skips the repack launch); bits 8-9: timing
 *            experiments only (skip MFMAs / gathers).
 *   wpack    float32 scratch, aabr_conv_wpack_floats(vol,nIn,nOut) elements                   */
int64_t aabr_conv_wpack_floats(int vol, int n_in, int n_out);
int aabr_conv_forward(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                      int64_t V_out, const int32_t *blocks, int vol, const float *W,
                      const float *bias, int flags, float *wpack, void *stream);
/* Training steps need W packed in both orientations once per weight version: this fills the forward
 * layout (what aabr_conv_forward builds for flags bit0 = 0) and the input-gradient layout (bit0 = 1)
 * in one launch; the conv calls then pass flags bit2.  Each pack holds
 * aabr_conv_wpack_floats(vol,nIn,nOut) elements (float32 / bf16 bit patterns).                   */
int aabr_conv_pack_weights2(const float *W, int vol, int n_in, int n_out, float *wpack_fwd,
                            float *wpack_t, void *stream);
int aabr_conv_pack_weights2_bf16(const float *W, int vol, int n_in, int n_out, uint16_t *wpack_fwd,
                                 uint16_t *wpack_t, void *stream);
/* All convolutions of a network in one launch.  jobs_dev: device array of n_jobs records of 48 bytes
 *   { const float *W; void *wpack_fwd; void *wpack_t; int32 vol, n_in, n_out, bf16; int64 first_block; }
 * first_block[j] = sum of aabr_conv_pack_job_blocks(...) of the jobs before j; total_blocks = that sum over
 * all jobs.  Same layouts as aabr_conv_pack_weights2[_bf16] (bf16 != 0: bf16 bit patterns).  The reference
 * has no counterpart: its GEMMs read W[k] in place (CPU/Convolution.cpp:60-66).                       */
int64_t aabr_conv_pack_job_blocks(int vol, int n_in, int n_out);
int aabr_conv_pack_weights_jobs(const void *jobs_dev, int n_jobs, int64_t total_blocks, void *stream);
/* dW[k] = sum over offset k's pairs (t, o) of in[t]^T (x) d_out[o]; d_bias (optional) = column
 * sums of d_out.  max_chunks bounds the number of chunks of c = aabr_conv_dw_chunk_pairs(V, vol, nIn, nOut) pairs:
 * sum_k ceil(R_k/c) when the rule counts are known on the host, else ceil(vol*V/c) + vol; scratch float32
 * [aabr_conv_dw_scratch_floats(max_chunks, nIn, nOut)].  Deterministic (no atomics).
 * Replaces the dW half of *_backward (CPU/Convolution.cpp:81-115,151-185;
 * CUDA/Convolution.cu:249-441,526-667).                                                     */
int64_t aabr_conv_dw_scratch_floats(int64_t max_chunks, int n_in, int n_out);
int aabr_conv_dw_chunk_pairs(int64_t V_out, int vol, int n_in, int n_out); /* 256 or 1024 */
/* Which operands' rows a launch with these arguments gathers with one 16- / 8-byte load per lane (fp32 storage, the
 * 64 x 64-block kernel; csrc/conv_dw_tiles.h dw_vec_operands): bit 0 the input features, bit 1 the output gradients; 0
 * for every other kernel and under the knob DW_VEC = 0.  The result of the launch does not depend on it.            */
int aabr_conv_dw_vec_operands(int bf16, const void *in_feats, int n_in, const void *d_out, int n_out, int64_t V_out,
                              int vol, int64_t max_chunks);
int aabr_conv_backward_weight(const float *in_feats, int n_in, const float *d_out, int n_out,
                              int64_t V_out, const int32_t *pairs, int vol, int64_t max_chunks,
                              float *dW, float *d_bias, float *scratch, void *stream);

/* ---- batch normalisation + leaky ReLU ------------------------------------------------------
 * Replaces BatchNormalization_updateOutput / _backward (SCN/CPU/BatchNormalization.cpp:12-157,
 * SCN/CUDA/BatchNormalization.cu:14-238).  weight/bias may be NULL.  scratch: float32
 * [aabr_bn_scratch_floats(planes)].                                                         */
int64_t aabr_bn_scratch_floats(int planes);
int aabr_bn_forward(const float *in, float *out, int64_t rows, int planes, float *save_mean,
                    float *save_invstd, float *running_mean, float *running_var,
                    const float *weight, const float *bias, float eps, float momentum,
                    int train, float leakiness, float *scratch, void *stream);
/* backward: `bias` is the forward pass's bias (as the reference's BatchNormalization_backward receives it,
 * pybind.cpp:219-221).  fp32 storage with leakiness >= 0 derives the activation mask from in, save_mean,
 * save_invstd, weight and bias (bit-identical to reading it from `out`, which may then be NULL).       */
int aabr_bn_backward(const float *in, float *d_in, const float *out, const float *d_out,
                     int64_t rows, int planes, const float *save_mean, const float *save_invstd,
                     const float *weight, const float *bias, float *d_weight, float *d_bias, float leakiness,
                     float *scratch, void *stream);

/* the same with d_in = BatchNorm gradient + d_in_add ([rows, planes] fp32, may be NULL): the gradient sum autograd
 * forms for a tensor with a second consumer (identity branch of a residual block, lateral connection) folded into
 * the apply pass.                                                                                       */
int aabr_bn_backward_add(const float *in, float *d_in, const float *out, const float *d_out, int64_t rows,
                         int planes, const float *save_mean, const float *save_invstd, const float *weight,
                         const float *bias, float *d_weight, float *d_bias, float leakiness, float *scratch,
                         const float *d_in_add, void *stream);

/* ---- bf16 feature storage (extension; BASELINE.json configs 3-5) ------------------------------
 * The reference instantiates its operators for float only (SCN/sparseconvnet_cuda.cpp:281-310).
 * These variants keep the SAME rule-book formats, fp32 parameters (W, bias, batch-norm affine and
 * statistics) and fp32/fp64 accumulation; only the [rows, planes] feature matrices (and their
 * gradients) are bfloat16, passed as uint16_t bit patterns.  Convolution: nIn % 32 == 0 and
 * nOut % 32 == 0 (v_mfma_f32_16x16x32_bf16 consumes one 32-plane chunk per instruction), every
 * buffer < 2 GiB; flags bits 0-2 as aabr_conv_forward; wpack = uint16
 * [aabr_conv_wpack_bf16_elems(vol,nIn,nOut)].  dW / d_bias stay fp32.                           */
int64_t aabr_conv_wpack_bf16_elems(int vol, int n_in, int n_out);
int aabr_conv_forward_bf16(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats,
                           int n_out, int64_t V_out, const int32_t *blocks, int vol, const float *W,
                           const float *bias, int flags, uint16_t *wpack, void *stream);
/* bf16 storage through the wide-layer kernel (128-row tiles, columns split over the waves, gathered rows shared
 * through LDS): n_in % 64 == 0 (above 256: % 256), n_out % 64 == 0; the block stream is the fp32 wide kernel's
 * (aabr_build_wide_blocks), the weight pack aabr_conv_pack_weights2_bf16's.                              */
int aabr_conv_wide_tile_rows_bf16(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol);
int aabr_conv_forward_wide_bf16(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats, int n_out,
                                int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                                int flags, const uint16_t *wpack, void *stream);
int aabr_conv_backward_weight_bf16(const uint16_t *in_feats, int n_in, const uint16_t *d_out,
                                   int n_out, int64_t V_out, const int32_t *pairs, int vol,
                                   int64_t max_chunks, float *dW, float *d_bias, float *scratch,
                                   void *stream);
int aabr_bn_forward_bf16(const uint16_t *in, uint16_t *out, int64_t rows, int planes,
                         float *save_mean, float *save_invstd, float *running_mean,
                         float *running_var, const float *weight, const float *bias, float eps,
                         float momentum, int train, float leakiness, float *scratch, void *stream);
int aabr_bn_backward_bf16(const uint16_t *in, uint16_t *d_in, const uint16_t *out,
                          const uint16_t *d_out, int64_t rows, int planes, const float *save_mean,
                          const float *save_invstd, const float *weight, const float *bias, float *d_weight,
                          float *d_bias, float leakiness, float *scratch, void *stream);
/* aabr_bn_backward_add for bf16 storage: d_in = bf16(bf16(BatchNorm gradient) + d_in_add); parts / nparts as
 * aabr_bn_backward_parts_bf16, or NULL / 0.                                                                        */
int aabr_bn_backward_add_bf16(const uint16_t *in, uint16_t *d_in, const uint16_t *out, const uint16_t *d_out,
                              int64_t rows, int planes, const float *save_mean, const float *save_invstd,
                              const float *weight, const float *bias, float *d_weight, float *d_bias, float leakiness,
                              const double *parts, int nparts, float *scratch, const uint16_t *d_in_add, void *stream);

/* ---- the proposal stage of a whole batch (extension) --------------------------------------------
 * The reference's RPNPostProcessor loops over the examples in Python (rpn/inference_3d.py:95-149).
 * aabr_rpn_gather_logits: out[b][j] = j-th logit of example b's cross-scale anchor list (maps in order; tables
 *   [nb][n_maps+1] / [nb][n_maps] on the host as for aabr_rpn_decode_maps), -inf from its end to lmax -- one
 *   top-k over dim 1 then selects for every example.  A NaN logit is written as the quiet NaN with the sign bit
 *   clear (0x7fc00000), which torch.topk on the device puts first like aabr_rpn_topk_maps does; one with the sign bit
 *   set it would select but sort last.
 * aabr_rpn_proposals_batch: per example aabr_rpn_decode_maps on selected[b] followed by aabr_rotate_nms_sorted of
 *   the decoded list; boxes / nms_boxes [nb,k,7], scores [nb,k], mask [nb][k*ceil(k/64)], keep [nb,k],
 *   meta [nb][AABR_META_WORDS] (meta[b][0] = number kept, left on the device).  At most 8 maps, 16 examples.  */
/* aabr_rpn_topk_maps (round 5): the per-example `objectness.topk(pre_nms_top_n, sorted=True)` of RPNPostProcessor
 *   (rpn/inference_3d.py:107-112) for ALL examples of a step in four launches, on the logits (sigmoid is monotone), with
 *   nothing concatenated: selected[b][0..k_host[b]) = indices into example b's cross-scale anchor list (tables as for
 *   aabr_rpn_gather_logits) in torch.topk's value order, equal logits by ascending index: a NaN (either sign bit) ranks
 *   above +inf, then descending value with -0 equal to +0; logits that compare equal, and NaN among themselves, come
 *   out by ascending index, in the list and at the cut.  info[2b] = candidates gathered,
 *   info[2b+1] != 0: more than 4096 logits share the 24-bit prefix at the cut (exact ties en masse) -- selected[b] is then
 *   not valid (every entry still lies inside the list) and the caller falls back to a full sort.  k <= 2048.
 *   scratch: aabr_rpn_topk_scratch_words(nb) int32.  */
int64_t aabr_rpn_topk_scratch_words(int nb);
int aabr_rpn_topk_maps(int n_maps, const void *const *logit_ptrs, int nb, const int32_t *seg_begin_host,
                       const int32_t *site_begin_host, int num_anchors, const int32_t *k_host, int64_t *selected,
                       int64_t sel_stride, int32_t *info, int32_t *scratch, void *stream);
int aabr_rpn_gather_logits(int n_maps, const void *const *logit_ptrs, int nb, const int32_t *seg_begin_host,
                           const int32_t *site_begin_host, int num_anchors, int64_t lmax, float *out, void *stream);
int aabr_rpn_proposals_batch(int n_maps, const void *const *coords_ptrs, const void *const *logit_ptrs,
                             const void *const *regression_ptrs, int nb, const int32_t *seg_begin_host,
                             const int32_t *site_begin_host, const float *strides_host, const float *base_anchors,
                             int num_anchors, float voxel_scale, const float *weights_host, float clip,
                             float nms_min_yx, float nms_min_z, const int64_t *selected, int64_t k, float *boxes,
                             float *nms_boxes, float *scores, float nms_thresh, int only_xy, int64_t post_max,
                             uint64_t *mask, int64_t *keep, int32_t *meta, void *stream);

/* Offset split of the wide kernel for coarse maps (extension; same contraction, same results up to the summation
 * order over filter offsets, which is fixed: part order): when a layer has too few (tile, 64-column slab) items to
 * fill the chip -- the coarse FPN scales -- every item is cut into `parts` workgroups, each sweeping vol / parts filter
 * offsets into its own fp32 partial tile in `scratch` (parts x V_out x n_out floats, 16-byte aligned); a second launch
 * adds the parts in part order, then bias and residual.  aabr_conv_wide_split returns (parts << 16) | tile_rows when
 * a launch should take this path (asked after aabr_conv_wide_tile_rows returned 0), else 0; blocks =
 * aabr_build_wide_blocks(.., tile_rows).  fp32 storage.                                                        */
int aabr_conv_wide_split(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol);
int64_t aabr_conv_wide_split_scratch_floats(int64_t V_out, int n_out, int parts);
int aabr_conv_forward_wide_split(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                                 int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                                 int flags, const float *wpack, const float *residual, int parts, float *scratch,
                                 void *stream);

/* the same for bf16 feature storage (in / out / wpack bf16, parts fp32, one rounding in the second stage; the residual
 * form is aabr_conv_forward_wide_split_bf16_res below) */
int aabr_conv_wide_split_bf16(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol);
int aabr_conv_forward_wide_split_bf16(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats, int n_out,
                                      int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                                      int flags, const uint16_t *wpack, int parts, float *scratch, void *stream);
/* ... with `residual` (bf16 [V_out, n_out], may be NULL): out = bf16(bf16(sum of the parts + bias) + residual), what the
 * separate bf16 add of the consumer would have stored.                                                                */
int aabr_conv_forward_wide_split_bf16_res(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats,
                                          int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                          const float *bias, int flags, const uint16_t *wpack, int parts, float *scratch,
                                          const uint16_t *residual, void *stream);

/* 32 -> 32 plane layers (the finest scales; csrc/conv_narrow.hip): the same sum as aabr_conv_forward (Convolution.cpp:
 * 117-185), read from the GATHER TABLE `table` [vol][V_out] (input row of output row o at offset k, or -1 -- what
 * aabr_submanifold_table / aabr_convolution_tables leave behind) instead of a block stream, with the fp32 master weights
 * W [vol][32][32] staged in LDS by the launch itself (no pack call).  flags: bit 0 transposed weights, bit 1 mirrored
 * offsets (the submanifold input-gradient form).  aabr_conv_narrow_ok: 1 when the dispatch hands a launch to it (bf16
 * storage from 400,000 output rows on: where the tile kernels' per-block weight stream stops fitting the L2s).       */
int aabr_conv_narrow_ok(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, int bf16);
int aabr_conv_forward_narrow(const float *in_feats, int64_t rows_in, float *out_feats, int64_t V_out, const int32_t *table,
                             int vol, const float *W, const float *bias, int flags, void *stream);
int aabr_conv_forward_narrow_bf16(const uint16_t *in_feats, int64_t rows_in, uint16_t *out_feats, int64_t V_out,
                                  const int32_t *table, int vol, const float *W, const float *bias, int flags, void *stream);
/* ... with the BatchNorm statistics of the write-out, one [2][32] fp64 pair per workgroup of the launch
 * (aabr_conv_narrow_parts(V_out) of them): forward sums of the stored values (consumer aabr_bn_forward_parts_bf16) /
 * backward sums of the BatchNorm whose d_out the launch writes (consumer aabr_bn_backward_parts_bf16), as the wide kernel's
 * aabr_conv_forward_wide_bf16_stats / _bwd_stats form them per tile. */
int aabr_conv_narrow_parts(int64_t V_out);
int aabr_conv_forward_narrow_bf16_stats(const uint16_t *in_feats, int64_t rows_in, uint16_t *out_feats, int64_t V_out,
                                        const int32_t *table, int vol, const float *W, const float *bias, int flags,
                                        double *stats, void *stream);
int aabr_conv_forward_narrow_bf16_bwd_stats(const uint16_t *in_feats, int64_t rows_in, uint16_t *out_feats, int64_t V_out,
                                            const int32_t *table, int vol, const float *W, const float *bias, int flags,
                                            double *stats, const uint16_t *bn_in, const uint16_t *bn_out,
                                            const float *save_mean, float leakiness, void *stream);

/* ---- compiled launch plans (extension) --------------------------------------------------------
 * The reference enters its library once per layer and direction from Python (SCN/pybind.cpp:134-221 behind
 * sparseconvnet/ layer modules).  A host that has compiled the static part of a network into a list of launches hands
 * the whole list over with ONE call: every record stands for one of the entry points above, called with the
 * record's fields in the order given here -- nothing is computed differently.
 *   kind AABR_PLAN_CONV       aabr_conv_forward[_bf16](p0 in, i32[0] n_in, i64[0] rows_in, p1 out, i32[1] n_out,
 *                             i64[1] V_out, p2 blocks, i32[2] vol, p3 W, p4 bias, i32[3] flags, p5 wpack)
 *        AABR_PLAN_CONV_WIDE  aabr_conv_forward_wide_stats(p0, i32[0], i64[0], p1, i32[1], i64[1], p2 blocks,
 *                             i32[4] tile_rows, i32[2] vol, p4 bias, i32[3] flags, p5 wpack, p3 residual, p6 stats),
 *                             the forward statistics of the FOLLOWING BatchNorm (p6 NULL: none; p7 .. p11 must be NULL);
 *                             i32[5] == 1: aabr_conv_forward_wide_bwd_stats(..., p3 residual, p6 stats, p7 bn_in,
 *                             p8 save_mean, p9 save_invstd, p10 bn_weight, p11 bn_bias, f32[0] leakiness); bf16
 *                             storage: aabr_conv_forward_wide_bf16_res(..., p5 wpack, p3 residual, p6 stats), with
 *                             i32[5] == 1 also p7 bn_in, p9 bn_out, p8 save_mean, f32[0] leakiness (the backward
 *                             statistics); p3 / p6 NULL: no residual / no statistics, in either storage -- in bf16
 *                             storage too p3 is READ as the residual (bf16 rows): it must be NULL when none is wanted
 *        AABR_PLAN_CONV_DW    aabr_conv_backward_weight[_bf16](p0 in, i32[0] n_in, p1 d_out, i32[1] n_out,
 *                             i64[0] V_out, p2 pairs, i32[2] vol, i64[1] max_chunks, p3 dW, p4 d_bias, p5 scratch)
 *        AABR_PLAN_BN_FWD     aabr_bn_forward[_bf16](p0 in, p1 out, i64[0] rows, i32[0] planes, p2 save_mean,
 *                             p3 save_invstd, p4 running_mean, p5 running_var, p6 weight, p7 bias, f32[0] eps,
 *                             f32[1] momentum, i32[1] train, f32[2] leakiness, p8 scratch); p9 != NULL:
 *                             aabr_bn_forward_parts[_bf16](..., p9 parts, i32[2] nparts, p8 scratch)
 *        AABR_PLAN_BN_BWD     aabr_bn_backward[_bf16](p0 in, p1 d_in, p2 out, p3 d_out, i64[0] rows, i32[0] planes,
 *                             p4 save_mean, p5 save_invstd, p6 weight, p10 bias, p7 d_weight, p8 d_bias,
 *                             f32[2] leakiness, p9 scratch) with p11 d_in_add (the gradient sum folded in; NULL: none,
 *                             in either storage) and, i64[1] != 0, the statistics' partial sums (parts =
 *                             (double *)i64[1], i32[1] nparts).  A bf16 record's p11 is READ and added as a fp32 one's
 *                             is: it must be NULL when no sum is wanted.  fp32: i64[1] != 0 ?
 *                             aabr_bn_backward_parts(..., p9, p11) : aabr_bn_backward_add(..., p9, p11); bf16: p11 != NULL ?
 *                             aabr_bn_backward_add_bf16(..., parts or NULL, i32[1], p9, p11) : i64[1] != 0 ?
 *                             aabr_bn_backward_parts_bf16(..., parts, i32[1], p9) : aabr_bn_backward_bf16(..., p9)
 *        AABR_PLAN_ADD        aabr_add(p0 a, p1 b, p2 out, i64[0] n)
 *        AABR_PLAN_CAST       aabr_cast_storage(p0 in, p1 out, i64[0] n, flags & AABR_PLAN_TO_BF16)
 *   flags & AABR_PLAN_BF16 selects the bf16-storage entry point.  Stops at the first failing record and returns
 *   its code (aabr_last_error() holds that entry point's message).                                    */
#define AABR_PLAN_CONV 1
#define AABR_PLAN_CONV_WIDE 2
#define AABR_PLAN_CONV_DW 3
#define AABR_PLAN_BN_FWD 4
#define AABR_PLAN_BN_BWD 5
#define AABR_PLAN_ADD 6
#define AABR_PLAN_CAST 7
#define AABR_PLAN_CONV_WIDE_SPLIT 9 /* aabr_conv_forward_wide_split(p0, i32[0], i64[0], p1, i32[1], i64[1], p2 blocks,
                                       i32[4] tile_rows, i32[2] vol, p4 bias, i32[3] flags, p5 wpack, p3 residual,
                                       i32[5] parts, p6 scratch); bf16 storage: aabr_conv_forward_wide_split_bf16_res(
                                       ..., p3 residual); p3 NULL: no residual, in either storage (a bf16 record's
                                       p3 is read as bf16 rows: it must be NULL when no residual is wanted) */
#define AABR_PLAN_CONV_NARROW 10 /* aabr_conv_forward_narrow[_bf16](p0 in, i64[0] rows_in, p1 out, i64[1] V_out, p2 table,
                                   i32[2] vol, p3 W (the raw weight: this kernel takes no residual), p4 bias,
                                   i32[3] flags); bf16 storage with p6 != NULL: .._bf16_stats(.., p6 stats); bf16
                                   storage with i32[5] == 1: .._bf16_bwd_stats(.., p6 stats, p7 bn_in, p9 bn_out,
                                   p8 save_mean, f32[0] leakiness); fp32 storage reads neither: p6 .. p11 must be NULL */
#define AABR_PLAN_CONV_SINGLE 11 /* aabr_conv_forward_single(p0 in, i32[0] n_in, i64[0] rows_in, p1 out, i32[1] n_out,
                                   i64[1] V_out, p2 pairs, i32[2] vol, p4 bias, i32[3] flags, p5 wpack, p3 residual);
                                   fp32 storage only; the caller guarantees one rule per output row; p3 NULL: no
                                   residual.  i32[5] == 1: aabr_conv_forward_single_bwd_stats(..., p3 residual,
                                   p6 stats, p7 bn_in, p8 save_mean, p9 save_invstd, p10 bn_weight, p11 bn_bias,
                                   f32[0] leakiness); otherwise p6 .. p11 are not read and must be NULL */
#define AABR_PLAN_BF16 1
#define AABR_PLAN_TO_BF16 2
#define AABR_PLAN_JOIN 8 /* the caller's stream waits for the second stream in front of this record */
#define AABR_PLAN_SIDE 4 /* run this record on the library's second stream: it starts after everything recorded
                            before it, and the caller's stream waits for it before aabr_plan_run returns it */
/* The deferred-join TAIL (extension): launches whose results nothing later in the list and no returned buffer reads.
 *   AABR_PLAN_TAIL (flag)  the record runs on the library's tail stream (process-wide, one per device, lowest stream
 *                          priority), in list order among the tail records.  A run of consecutive tail records starts
 *                          after everything recorded before its first record on the caller's stream (one event per
 *                          run).  It is NOT joined when the call returns: only aabr_plan_run_tail accepts such records,
 *                          and hands back a ticket.  aabr_plan_run and aabr_plan_submit refuse them (AABR_EINVAL).
 *                          Cannot be combined with AABR_PLAN_SIDE / AABR_PLAN_JOIN.  Runs of AABR_PLAN_CAST records are
 *                          merged per stream: a tail cast never joins a run of the caller's stream.
 *   ticket                 an event recorded behind the last tail record of the call; 0 = the list had no tail record
 *                          (or PLAN_TAIL = 0).  The CALLER owns it, from the moment aabr_plan_run_tail returns AABR_OK
 *                          until it calls aabr_plan_tail_release; on any other return code no tail is left running
 *                          (the call has synchronised it) and the ticket is 0.
 *   who must join before what: the holder makes a stream wait for the ticket -- aabr_plan_tail_join(ticket, stream),
 *                          or an AABR_PLAN_TAIL_JOIN record (kind; i64[0] = the ticket, every other field 0) in a list
 *                          run on that stream -- BEFORE anything on that stream overwrites or frees what the tail
 *                          reads or writes: its operands, scratch buffers, the parameters and running statistics an
 *                          optimizer step or a later pass rewrites.  aabr_plan_tail_sync(ticket) is the host-side form.
 *                          All three may be called from any thread, any number of times; for ticket 0 and for a
 *                          RELEASED ticket they do nothing and return AABR_OK (releasing says "I have joined").
 *   aabr_plan_tail_release returns the ticket's event to the library's pool; a second release does nothing.  Release
 *                          only after a join has been enqueued (or a sync has returned): the library does not wait.
 *   PLAN_TAIL knob         0 = tail records run where they stand in the list on the caller's stream, ticket 0;
 *                          1 = the tail stream is a stream of its own; 2 = the tail stream IS the second stream, one
 *                          per process and device, shared with the AABR_PLAN_SIDE records of every thread (a process
 *                          has a fixed number of hardware queues; with 1 the side stream stays per thread). */
#define AABR_PLAN_TAIL 16
#define AABR_PLAN_TAIL_JOIN 12
typedef struct AabrPlanOp {
  int32_t kind, flags;
  int32_t i32[6];
  float f32[4];
  int64_t i64[4];
  void *p[12];
} AabrPlanOp; /* 176 bytes, no padding */
int aabr_plan_run(const AabrPlanOp *ops, int n_ops, void *stream);
int aabr_plan_run_tail(const AabrPlanOp *ops, int n_ops, void *stream, uint64_t *ticket);
int aabr_plan_tail_join(uint64_t ticket, void *stream);
int aabr_plan_tail_sync(uint64_t ticket);
int aabr_plan_tail_release(uint64_t ticket);
/* Pipelined form (extension): a pass's list handed over in PARTS.  aabr_plan_submit copies the records, queues them for the
 * library's launcher thread and returns at once -- the caller fills the next part while this one's launches go out
 * (issuing ~450 launches costs the host 1.7 ms per training step, filling their records about as much).  Parts are
 * issued strictly in submission order with the semantics of aabr_plan_run; with hold_side != 0 the part leaves the
 * second stream unjoined for the part that follows (the last part of a pass passes 0).  aabr_plan_drain blocks until
 * every submitted part has been ISSUED and returns the first failing part's code (aabr_last_error() holds its
 * message): call it before enqueuing anything else on the streams used.  The failure is STICKY: from the failing part
 * on every submitted part -- of this pass or of a later one -- is dropped until aabr_plan_drain has returned the code.
 * aabr_plan_run refuses to run while submitted parts are queued or being issued (AABR_EINVAL); after the drain
 * aabr_conv_last_variant() on the calling thread names what the drained parts dispatched last. */
int aabr_plan_submit(const AabrPlanOp *ops, int n_ops, void *stream, int hold_side);
int aabr_plan_drain(void);
/* (tools) the launcher's counters since process start: time spent issuing parts, parts issued, times it found its
 * queue empty */
void aabr_plan_launcher_stats(int64_t *busy_ns, int64_t *parts, int64_t *sleeps);
/* Geometry plan (extension): the rule-book builders of a pass handed over as ONE list, each record = one of the
 * entry points above called with the record's fields -- nothing is computed differently:
 *   AABR_GEOM_SUBM_TABLE    aabr_submanifold_table(p0 coords, i64[0] V, p1 grid, i64[1] cap, i32[0..2] filter,
 *                           p2 table, p3 counts)
 *   AABR_GEOM_CONV_TABLES   aabr_convolution_tables2(p0 in_coords, i64[0] V_in, p1 in_grid, i64[1] in_cap,
 *                           p2 out_coords, i64[2] V_out, p3 out_grid, i64[3] out_cap, i32[0..2] size,
 *                           i32[3..5] stride, i32[6..8] out_spatial, p4 table_out, p5 table_in, p6 counts, p7 counts_in)
 *   AABR_GEOM_TILE_BLOCKS   aabr_build_tile_blocks(p0 table, i64[0] V, i32[0] vol, p1 blocks)
 *   AABR_GEOM_WIDE_BLOCKS   aabr_build_wide_blocks(p0 table, i64[0] V, i32[0] vol, i32[1] tile_rows, p1 blocks)
 *   AABR_GEOM_OFFSET_PAIRS  aabr_build_offset_pairs(p0 table, p1 block_counts, i64[0] V, i32[0] vol, p2 pairs)
 *   AABR_GEOM_CONV_SITES    aabr_convolution_sites(p0 in_coords, i64[0] V_in, i32[0..2] size, i32[3..5] stride,
 *                           i32[6..8] out_spatial, p1 out_grid, i64[1] out_cap, p2 scratch, p3 out_coords, p4 meta)
 *   AABR_GEOM_SAMPLE_OFFSETS aabr_sample_offsets(p0 coords, p1 meta, i64[0] V_max, i32[0] max_samples, p2 out)
 * Stops at the first failing record and returns its code.                                                      */
#define AABR_GEOM_SUBM_TABLE 1
#define AABR_GEOM_CONV_TABLES 2
#define AABR_GEOM_TILE_BLOCKS 3
#define AABR_GEOM_WIDE_BLOCKS 4
#define AABR_GEOM_OFFSET_PAIRS 5
#define AABR_GEOM_CONV_SITES 7
#define AABR_GEOM_SAMPLE_OFFSETS 8
/* brick grids (one allocation per level: the directory, then the bricks; dims packed sbx | sby << 16 | sbz << 32 | nb << 48):
 *   AABR_GEOM_BRICK_BUILD   aabr_brick_build(p0 in_coords, i64[0] vin_bound, p1 vin_count_dev, i32[0..2] size, i32[3..5]
 *                           stride, i32[6..8] out_spatial, i64[1] dims, p2 level, i64[2] nb_cap, p3 bcoord, p4 out_coords,
 *                           i64[3] v_cap, p5 meta, p6 scratch, i32[9] flags)
 *   AABR_GEOM_BRICK_SUBM    aabr_brick_submanifold_table(p0 coords, i64[0] V, i64[1] dims, p1 level, i32[0..2] filter,
 *                           p2 table, p3 block counts)
 *   AABR_GEOM_BRICK_TABLES  aabr_brick_convolution_tables(p0 in_coords, i64[0] V_in, i64[2] in dims, p1 in level,
 *                           p2 out_coords, i64[1] V_out, i64[3] out dims, p3 out level, i32[0..2] size, i32[3..5] stride,
 *                           i32[6..8] out_spatial, p4 table_out, p5 table_in, p6 counts, p7 counts_in)                  */
#define AABR_GEOM_BRICK_BUILD 9
#define AABR_GEOM_BRICK_SUBM 10
#define AABR_GEOM_BRICK_TABLES 11
typedef struct AabrGeomOp {
  int32_t kind, pad;
  int32_t i32[10];
  int64_t i64[4];
  void *p[8];
} AabrGeomOp; /* 144 bytes, no padding */
int aabr_geom_run(const AabrGeomOp *ops, int n_ops, void *stream);

/* Mailbox (extension): a small result (counts the host needs to size the next launches) handed over WITHOUT a stream or
 * event wait on the receiving side.  aabr_mailbox_create: coherent pinned host memory, [0] = sequence word (starts 0),
 * [1] reserved, payload from byte 8.  aabr_mailbox_post (one small kernel on `stream`): copies `bytes` (% 4) from
 * device memory into the payload, then stores `seq` (!= 0) into the sequence word with a system-scope release; the
 * host spins on that word and then reads the payload.  Why: hipStreamSynchronize / hipEventSynchronize / polling
 * hipEventQuery on the producing stream were measured to return only when the process's OTHER streams had drained
 * (csrc/plan.hip, profiles/r03_step_timeline.txt).  One post in flight per mailbox.                             */
int aabr_mailbox_create(int64_t payload_bytes, void **box);
int aabr_mailbox_destroy(void *box);
int aabr_mailbox_post(const void *src, int64_t bytes, void *box, uint32_t seq, void *stream);

/* out = a + b elementwise over n elements (fp32, or bf16 storage with the sum formed in fp32 and rounded to
 * nearest even); fp32 <-> bf16 storage cast.  What the layer API gets from torch (`a + b`, `.to(dtype)`; the
 * reference: AddTable, tables.py:27-41) as plan records.                                           */
int aabr_add(const void *a, const void *b, void *out, int64_t n, int bf16, void *stream);
int aabr_cast_storage(const void *in, void *out, int64_t n, int to_bf16, void *stream);
/* out_host[j][0] = sum of the n_host[j] int32 values at counts_host[j], for n_jobs rule books in one launch (the
 * host arrays hold DEVICE pointers).  The reference returns the rule total of a layer from host memory
 * (`forward_pass_multiplyAdd_count`, submanifoldConvolution.py:85-94); here the per-block rule counts live on the
 * device and the totals are kept there until somebody reads the counter.                             */
int aabr_sum_counts(const int32_t *const *counts_host, const int64_t *n_host, double *const *out_host, int n_jobs,
                    void *stream);

/* ---- rotated IoU / NMS ---------------------------------------------------------------------
 * iou[n,k] = devRotateIoUEval(query k, box n, criterion), then forced to 1 where the five
 * parameters differ by < 1e-6 -- rotate_iou_gpu_eval + check_same_boxes
 * (second/core/non_max_suppression/nms_gpu.py:552-717).  boxes [N,5], query [K,5]
 * = (xc, yc, size_a, size_b, yaw).                                                           */
int aabr_rotate_iou_eval(const float *boxes, int64_t N, const float *query, int64_t K,
                         int criterion, float *iou, void *stream);
/* boxes_iou_3d (utils3d/rotate_nms_3d_torch.py:23-90) on [.,7] yx_zb boxes;
 * aug_host[4] = {target_Y, target_Z, anchor_Y, anchor_Z}.                                    */
int aabr_boxes_iou_3d(const float *targets, int64_t M, const float *anchors, int64_t K,
                      const float *aug_host, int criterion, int only_xy, float *iou,
                      void *stream);
/* RPN label generation, fused and batched over the examples of a step.  Per example b and per
 * anchor of its concatenated list [map][site][yaw] (maps / segment tables as in aabr_rpn_decode_maps, one row of
 * seg_begin_host [nb][n_maps+1] and site_begin_host [nb][n_maps] per example): the IoU with every ground-truth box of
 * the example -- boxlist_iou_3d(target, anchor, aug_thickness, criterion, flag='rpn_label_generation'),
 * modeling/rpn/loss_3d.py:91-96, i.e. aabr_boxes_iou_3d on the anchors of anchor_generator_sparse3d.py:88-104 --
 * and Matcher.__call__ as make_rpn_loss_evaluator builds and calls it (modeling/rpn/loss_3d.py:96-100,338-344;
 * modeling/matcher.py:50-196): the entries whose |yaw difference| (utils3d/geometric_torch.py:4-21, target - anchor
 * wrapped to [-pi/2, pi/2)) is not below yaw_threshold are zeroed (no mask when yaw_threshold > 1.58, matcher.py:51);
 * matched_val = best masked value over the ground truths, matched_idx = its index (first maximum), or -1 below
 * bg_iou / -2 below fg_iou; with allow_low_quality_matches != 0 (the RPN's setting) set_low_quality_matches_
 * follows: an anchor that ties with the row maximum of any ground truth gets its best index back, and an anchor
 * still at -1 with an entry above max(0.02, row maximum - 0.05) of any ground truth becomes -2.  A NaN entry (0 / 0 in
 * the z factor with only_xy off, or a non-finite box) behaves as in torch.max: it is its anchor's best value, the first
 * one by index, matched_val is NaN and the anchor is matched to that box; its ground truth's row maximum is NaN, which
 * ties with nothing.  All -1 for an
 * example without ground truth.  Outputs are concatenated over the examples in order (sum_b N_b entries); iou_out
 * (optional, may be NULL) receives the UNMASKED [G_b, N_b] IoU matrices back to back.  target_ptrs[b] = device
 * [G_b, 7] yx_zb boxes; aug_host[4] = {target_Y, target_Z, anchor_Y, anchor_Z}; row_max_scratch = device words,
 * sum_b G_b of them (needed with allow_low_quality_matches; the call clears them itself).                      */
int aabr_rpn_label_generation(int n_maps, const void *const *coords_ptrs, int nb, const int32_t *seg_begin_host,
                              const int32_t *site_begin_host, const float *strides_host, const float *base_anchors,
                              int num_anchors, float voxel_scale, const void *const *target_ptrs,
                              const int32_t *n_targets_host, const float *aug_host, int criterion, int only_xy,
                              float fg_iou, float bg_iou, float yaw_threshold, int allow_low_quality_matches,
                              int64_t *matched_idx, float *matched_val, float *iou_out, uint32_t *row_max_scratch,
                              void *stream);
/* The same call with the other half of RPNLossComputation.prepare_targets (modeling/rpn/loss_3d.py:186-196):
 * regression_targets [sum_b N_b, 7] (optional, may be NULL) = box_coder.encode(target[matched_idx.clamp(min=0)], anchor) for
 * EVERY anchor, in the pass that has the anchor and its match in registers -- BoxCoder3D.encode_centroid_box
 * (modeling/box_coder_3d.py:46-51): second_box_encode(., ., smooth_dim=True) (second/pytorch/core/box_torch_ops.py:82-116),
 * yaw difference through limit_period(., 0.5, pi), times weights_host[7]; the un-thickened anchor and ground-truth box.
 * An example without ground truth encodes every anchor against itself (loss_3d.py:91-94: matched_targets = anchor).   */
int aabr_rpn_label_generation_targets(int n_maps, const void *const *coords_ptrs, int nb, const int32_t *seg_begin_host,
                                      const int32_t *site_begin_host, const float *strides_host,
                                      const float *base_anchors, int num_anchors, float voxel_scale,
                                      const void *const *target_ptrs, const int32_t *n_targets_host,
                                      const float *aug_host, int criterion, int only_xy, float fg_iou, float bg_iou,
                                      float yaw_threshold, int allow_low_quality_matches, int64_t *matched_idx,
                                      float *matched_val, float *iou_out, uint32_t *row_max_scratch,
                                      const float *weights_host, float *regression_targets, void *stream);
/* BoxCoder3D.encode (modeling/box_coder_3d.py:34-51, centroid form) on two [n,7] lists: out [n,7].                  */
int aabr_box_encode(const float *targets, const float *anchors, int64_t n, const float *weights_host, float *out,
                    void *stream);
/* BoxCoder3D.decode (modeling/box_coder_3d.py:40-44,53-80, centroid form): encodings [n, 7*num_classes] / weights, sizes
 * clamped at `clip` (bbox_xform_clip), second_box_decode with smooth_dim (box_torch_ops.py:118-154) against anchors [n,7]
 * (one anchor per row, shared by its classes), yaw through limit_period(., 0.5, pi): out [n, 7*num_classes].         */
int aabr_box_decode(const float *encodings, const float *anchors, int64_t n, int num_classes,
                    const float *weights_host, float clip, float *out, void *stream);
/* The corner form of the coder (MODEL.CORNER_ROI; csrc/corner_box.h holds the per-box functions, host + device), on lists,
 * one thread per box and no host read (the reference converts in a Python loop over boxes on the host).
 * Two-corner boxes are [x0, y0, x1, y1, z0, z1, thickness]: the end points of the bottom centre line along the length.
 *   aabr_box_to_2corners   Box3D_Torch.from_yxzb_to_2corners (utils3d/bbox3d_ops_torch.py:115-135): yx_zb [n,7] -> two
 *                          corners [n,7]; rotation in fp64 rounded once to fp32 as numpy does it, yaw + pi/2 == 0 takes
 *                          the unrotated branch, corner 0 is the end whose offset from the centroid has a component
 *                          sum > 0 (strict: a tie swaps).
 *   aabr_box_from_2corners Box3D_Torch.from_2corners_to_yxzb (:29-55,93-112): two corners [n,7] -> yx_zb [n,7] in the
 *                          fp32 operations of the torch expressions (asin in fp64, narrowed); yaw in [-pi/2, pi/2).
 *   aabr_box_encode_corner BoxCoder3D(True, w).encode (modeling/box_coder_3d.py:82-91) of yx_zb targets against yx_zb
 *                          anchors, both [n,7]: second_corner_box_encode with smooth_dim between their two-corner forms,
 *                          times weights_host[7].  A zero-length or zero-height anchor gives the IEEE inf / NaN.
 *   aabr_box_decode_corner BoxCoder3D(True, w).decode (:93-122): encodings [n, 7*num_classes] / weights, elements 3..5
 *                          clamped at `clip`, second_corner_box_decode with smooth_dim against the proposals' two corners
 *                          (anchors [n,7] yx_zb, one per row, shared by its classes), back to yx_zb [n, 7*num_classes]. */
int aabr_box_to_2corners(const float *boxes, int64_t n, float *out, void *stream);
int aabr_box_from_2corners(const float *corners, int64_t n, float *out, void *stream);
int aabr_box_encode_corner(const float *targets, const float *anchors, int64_t n, const float *weights_host, float *out,
                           void *stream);
int aabr_box_decode_corner(const float *encodings, const float *anchors, int64_t n, int num_classes,
                           const float *weights_host, float clip, float *out, void *stream);
/* RPN glue: anchors of the selected flat indices t = site*A + yaw, generated from
 * the sparse site coordinates (modeling/rpn/anchor_generator_sparse3d.py:88-104:
 * centroid = loc / voxel_scale * stride, + base anchor), fused with BoxCoder3D.decode_centroid_box
 * (modeling/box_coder_3d.py:53-80; second_box_decode with smooth_dim, box_torch_ops.py:118-154;
 * limit_period to [-pi/2, pi/2]).  site_coords int32 [V,4]; selected int64 [k] indices relative
 * to (site_begin, reg_begin) of one example; regression float32 [*,7]; base_anchors [A,7];
 * boxes float32 [k,7] out (yx_zb).                                                             */
int aabr_rpn_decode(const int32_t *site_coords, int64_t site_begin, const int64_t *selected, int64_t k,
                    const float *regression, int64_t reg_begin, const float *base_anchors,
                    int num_anchors, float voxel_scale, const float *stride_host,
                    const float *weights_host, float clip, float *boxes, void *stream);

/* Cross-scale RPN proposals front end -- what RPNPostProcessor.forward_for_single_feature_map
 * (modeling/rpn/inference_3d.py:82-163) does per example AFTER cat_scales_obj_reg (rpn_sparse3d.py:19-77)
 * regrouped the scales example-major: for the k selected (top-k by objectness) entries of the example's
 * concatenated anchor list [map][site][yaw] -- anchor from the site coordinates
 * (anchor_generator_sparse3d.py:88-104) -> BoxCoder3D.decode_centroid_box (box_coder_3d.py:53-80) ->
 * sigmoid of the logit (:113) -> the boxlist_nms_3d thickness clamps (structures/boxlist_ops_3d.py:42-44)
 * into an NMS-only copy.  Host tables (n_maps <= 8): device pointers of each map's site list [V_m,4] int32,
 * logits [V_m*A] and regression [V_m*A,7]; seg_begin_host[n_maps+1] = first local anchor index of each map in
 * this example's list; site_begin_host[n_maps] = this example's first site row in each map;
 * strides_host[n_maps*3]; base_anchors device [n_maps*A,7].  selected int64 [k] (descending score).
 * Every entry that takes these two tables checks them alike (csrc/anchor_list.h): a row starts at 0, is
 * non-decreasing and every segment is a multiple of num_anchors; otherwise AABR_EINVAL before any launch.
 * Outputs: boxes [k,7], nms_boxes [k,7] (may be NULL), scores [k] (may be NULL).                 */
int aabr_rpn_decode_maps(int n_maps, const void *const *coords_ptrs, const void *const *logit_ptrs,
                         const void *const *regression_ptrs, const int32_t *seg_begin_host,
                         const int32_t *site_begin_host, const float *strides_host,
                         const float *base_anchors, int num_anchors, float voxel_scale,
                         const float *weights_host, float clip, float nms_min_yx, float nms_min_z,
                         const int64_t *selected, int64_t k, float *boxes, float *nms_boxes, float *scores,
                         void *stream);

/* Greedy rotated NMS over boxes already sorted by descending score: rotate_nms_3d_cc
 * (second/core/non_max_suppression/nms_cpu.py:32-44) with the suppression rule of
 * spconv-1.x rotate_non_max_suppression_cpu (IoU(i,j) > 0 and >= thresh).
 *   boxes7 [n,7]; mask scratch uint64 [n * ceil(n/64)]; keep int64 [n] out (indices into the
 *   sorted list, ascending = descending score); meta[0] = number kept (<= post_max).         */
int aabr_rotate_nms_sorted(const float *boxes7, int64_t n, float thresh, int only_xy,
                           int64_t post_max, uint64_t *mask, int64_t *keep, int32_t *meta,
                           void *stream);
/* maskrcnn_benchmark `_C.nms` (csrc/nms.h:10-28, csrc/cpu/nms_cpu.cpp:5-75,
 * csrc/cuda/nms.cu:23-131): axis-aligned, +1 pixel convention; dets [n,4] sorted by
 * descending score by the caller; keep = indices into the sorted list.                       */
int aabr_nms_sorted(const float *dets4, int64_t n, float thresh, uint64_t *mask, int64_t *keep,
                    int32_t *meta, void *stream);

/* ---- SparseToDense + rotated 3-D ROI align ----------------------------------
 * SparseToDense_updateOutput / _updateGradInput (SCN/CPU/SparseToDense.cpp:7-87, pybind.cpp:124-133):
 * out float32 [batch, planes, X, Y, Z] (zero-filled here), out[b][p][(x*Y+y)*Z+z] = in[row][p].   */
int aabr_sparse_to_dense_forward(const int32_t *site_coords, int64_t V, const float *in_feats, int planes,
                                 const int32_t *spatial_host, int64_t batch_size, float *out,
                                 void *stream);
int aabr_sparse_to_dense_backward(const int32_t *site_coords, int64_t V, float *d_in_feats, int planes,
                                  const int32_t *spatial_host, const float *d_out, void *stream);
/* `_C.roi_align_rotated_3d_forward / _backward` (maskrcnn_benchmark/csrc/vision.cpp:19-20,
 * csrc/cuda/ROIAlignRotated3D_cuda.cu:89-346): input [B,C,H,W,Z], rois [n,8] = (batch, center_w,
 * center_h, center_z, width, height, zsize, theta in degrees), output [n,C,ph,pw,pz].  The backward
 * zero-fills grad_input and accumulates with fp32 atomics, as the reference does.
 * An ROI whose batch index is negative or >= batch_size names an empty sample (ROIAlignRotated3D crops the batch to the
 * last occupied sample): its outputs are zero, it adds nothing backward, and nothing outside the tensors is touched --
 * the same rule as the fused sparse form below.  `_forward` without a batch size is the entry point of ABI <= 620: it
 * applies the rule to negative indices only and takes every other index as valid; new callers use `_forward_batch`. */
int aabr_roi_align_rotated_3d_forward_batch(const float *input, const float *rois, int64_t num_rois,
                                            float spatial_scale, int batch_size, int channels, int height, int width,
                                            int zsize, int pooled_h, int pooled_w, int pooled_z, int sampling_ratio,
                                            float *output, void *stream);
int aabr_roi_align_rotated_3d_forward(const float *input, const float *rois, int64_t num_rois,
                                      float spatial_scale, int channels, int height, int width, int zsize,
                                      int pooled_h, int pooled_w, int pooled_z, int sampling_ratio,
                                      float *output, void *stream);
int aabr_roi_align_rotated_3d_backward(const float *grad_output, const float *rois, int64_t num_rois,
                                       float spatial_scale, int pooled_h, int pooled_w, int pooled_z,
                                       int batch_size, int channels, int height, int width, int zsize,
                                       int sampling_ratio, float *grad_input, void *stream);

/* ---- fused sparse ROI-align (never densify) -----------------------------------------
 * Same contract as sparse_3d_to_dense_2d + _C.roi_align_rotated_3d_* (tools_3d_2d.py:7-48,
 * ROIAlignRotated3D_cuda.cu:16-346) without the dense [B,C,X,Y,Z] tensor: `cellmap` int32
 * [B, height, width, zsize] over the occupied extent (max coordinate + 1 per axis) holds the site row or -1
 * (aabr_roi_cellmap fills it); forward gathers feature rows [V, C] directly (bit-identical to the dense
 * form), backward adds into d_feats [V, C] (zeroed here; fp32 atomics on active cells only).          */
int aabr_roi_cellmap(const int32_t *site_coords, int64_t V, const int32_t *extent_host, int batch_size,
                     int32_t *cellmap, void *stream);
int aabr_roi_align_rotated_3d_sparse_forward(const float *feats, int channels, const int32_t *cellmap,
                                             int batch_size, int height, int width, int zsize,
                                             const float *rois, int64_t num_rois, float spatial_scale,
                                             int pooled_h, int pooled_w, int pooled_z, int sampling_ratio,
                                             float *output, void *stream);
int aabr_roi_align_rotated_3d_sparse_backward(const float *grad_output, int channels, const int32_t *cellmap,
                                              int batch_size, int height, int width, int zsize,
                                              const float *rois, int64_t num_rois, float spatial_scale,
                                              int pooled_h, int pooled_w, int pooled_z, int sampling_ratio,
                                              int64_t V, float *d_feats, void *stream);
/* bf16 feature storage (same reference lines; mirrors aabr_roi_align_rotated_3d_sparse_forward / _backward).
 * _forward_bf16: `feats` points at bf16 rows [V, C], 4-byte aligned; each of the eight corner values is widened
 *   (exact), the arithmetic and the fp32 output are bit for bit the fp32 call's on the widened rows.
 * _backward_bf16: never accumulates in bf16.  The fp32 call runs into `accum_f32` (caller-provided fp32 [V, channels],
 *   zeroed here, fp32 atomics) and its sums are rounded once (nearest even) into d_feats_bf16 [V, channels]:
 *   1 memset + 2 launches.  Both pointers 4-byte aligned.                                                           */
int aabr_roi_align_rotated_3d_sparse_forward_bf16(const void *feats_bf16, int channels, const int32_t *cellmap,
                                                  int batch_size, int height, int width, int zsize,
                                                  const float *rois, int64_t num_rois, float spatial_scale,
                                                  int pooled_h, int pooled_w, int pooled_z, int sampling_ratio,
                                                  float *output, void *stream);
int aabr_roi_align_rotated_3d_sparse_backward_bf16(const float *grad_output, int channels, const int32_t *cellmap,
                                                   int batch_size, int height, int width, int zsize,
                                                   const float *rois, int64_t num_rois, float spatial_scale,
                                                   int pooled_h, int pooled_w, int pooled_z, int sampling_ratio,
                                                   int64_t V, float *accum_f32, void *d_feats_bf16, void *stream);

/* ---- multi-level ROI pooler (csrc/roi_pool.hip): Pooler.forward of the box head (modeling/poolers_3d.py:73-168)
 * with FPN2MLPFeatureExtractor.convert_metric_to_pixel (roi_box_feature_extractors.py:108-114) in front of it.
 * Forward = 2 launches (prepare, gather), backward = 1 memset + 1 launch, whatever the level count; no host read.
 *
 * aabr_roi_pool_prepare: boxes [N, 7] yx_zb, the nb scenes' rows concatenated (n_host[b] rows each, 1 <= nb <= 16) ->
 *   rois [N, 8] fp32 = (scene, p1, p0, p2 + p5 / 2, p3, p4, p5, yaw in degrees), p = box[0..5] * box_scale, yaw =
 *   limit_period(box[6] + pi / 2, 0, pi) (BoxList3D.convert('standard') + the constructor's limit_yaw,
 *   Pooler.convert_to_roi_format), and levels [N] int32 = LevelMapper_3d: argmin_l |scales[l] - sqrt(max(p3, p4)) /
 *   canonical_size|, the first minimum, a NaN first (a NaN or negative size: level 0).  The fp32 operations of the torch
 *   expressions in their order, as CPU torch evaluates them (true divisions).
 * aabr_roi_pool_forward: output [num_rois, channels, ph, pw, pz]; ROI n is gathered from level levels[n] exactly as
 *   aabr_roi_align_rotated_3d_sparse_forward would on that level (bit-identical).  A level with V == 0, and a level index
 *   outside [0, n_levels), give zeros; every output element is written.  A level with V > 0 needs 1 <= nb <= batch_size.
 * aabr_roi_pool_backward: d_feats_all [total_rows, channels] holds every level's gradient rows, level l at row
 *   row_offset (row_offset + V <= total_rows); zeroed here, then fp32 atomics on active cells only.                   */
typedef struct AabrRoiLevel {
  const float *feats;          /* [V, channels] fp32 feature rows of the level (unused when V == 0); the _bf16 entry
                                  points read this pointer as bf16 rows [V, channels], 4-byte aligned                */
  const int32_t *cellmap;      /* [nb, height, width, zsize] int32, aabr_roi_cellmap over the occupied extent        */
  int32_t height, width, zsize; /* the occupied extent                                                               */
  int32_t nb;                  /* samples the cell map covers: an ROI of scene >= nb names an empty sample           */
  int64_t V;                   /* active sites                                                                       */
  int64_t row_offset;          /* backward: first row of this level in d_feats_all                                   */
  float spatial_scale;
  int32_t reserved;
} AabrRoiLevel;
int aabr_roi_pool_prepare(const float *boxes, int nb, const int64_t *n_host, float box_scale, int n_levels,
                          const float *scales_host, float canonical_size, float *rois, int32_t *levels, void *stream);
int aabr_roi_pool_forward(const AabrRoiLevel *levels_desc_host, int n_levels, int channels, int batch_size,
                          const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h, int pooled_w,
                          int pooled_z, int sampling_ratio, float *output, void *stream);
int aabr_roi_pool_backward(const AabrRoiLevel *levels_desc_host, int n_levels, int channels, int batch_size,
                           const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h, int pooled_w,
                           int pooled_z, int sampling_ratio, const float *grad_output, float *d_feats_all,
                           int64_t total_rows, void *stream);
/* bf16 feature storage of every level (Pooler.forward as above; mirrors aabr_roi_pool_forward / _backward).
 * aabr_roi_pool_forward_bf16: AabrRoiLevel.feats point at bf16 rows; the output stays fp32 and is bit for bit
 *   aabr_roi_pool_forward's on the widened rows.
 * aabr_roi_pool_backward_bf16: aabr_roi_pool_backward into `accum_f32` (caller-provided fp32 [total_rows, channels]),
 *   then ONE rounding (nearest even) into d_feats_all_bf16 [total_rows, channels]: 1 memset + 2 launches, nothing is
 *   accumulated in bf16.  accum_f32 keeps the fp32 sums.  Both 4-byte aligned.                                       */
int aabr_roi_pool_forward_bf16(const AabrRoiLevel *levels_desc_host, int n_levels, int channels, int batch_size,
                               const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h, int pooled_w,
                               int pooled_z, int sampling_ratio, float *output, void *stream);
int aabr_roi_pool_backward_bf16(const AabrRoiLevel *levels_desc_host, int n_levels, int channels, int batch_size,
                                const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h, int pooled_w,
                                int pooled_z, int sampling_ratio, const float *grad_output, float *accum_f32,
                                void *d_feats_all_bf16, int64_t total_rows, void *stream);
/* bf16 storage of the POOLED tensor and of its gradient (the same kernel, the pooled side's storage a template
 * parameter); feats_bf16 = 0 / 1 tells the storage of AabrRoiLevel.feats, as the two pairs above.
 * aabr_roi_pool_forward_pooled_bf16: output_bf16 [num_rois, channels, ph, pw, pz] in bf16 = ONE rounding (nearest even)
 *   of each fp32 value aabr_roi_pool_forward / _forward_bf16 stores; the zeros of a missing level are bf16 zeros; every
 *   element is written.                                                                                  1 launch.
 * aabr_roi_pool_backward_pooled_bf16: grad_output_bf16 in the same layout is widened on load (exact); atomics, their
 *   operands and the fp32 accumulation into accum_f32 [total_rows, channels] are aabr_roi_pool_backward's.
 *   feats_bf16 = 0: accum_f32 is the result, d_feats_all_bf16_or_null is not read.            1 memset + 1 launch.
 *   feats_bf16 = 1: the sums are rounded once into d_feats_all_bf16_or_null [total_rows, channels], as
 *   aabr_roi_pool_backward_bf16 does.                                                       1 memset + 2 launches.
 * A null pointer, or a bf16 pointer that is not 4-byte aligned, is AABR_EINVAL before any launch.                    */
int aabr_roi_pool_forward_pooled_bf16(const AabrRoiLevel *levels_desc_host, int n_levels, int channels, int batch_size,
                                      const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h,
                                      int pooled_w, int pooled_z, int sampling_ratio, int feats_bf16, void *output_bf16,
                                      void *stream);
int aabr_roi_pool_backward_pooled_bf16(const AabrRoiLevel *levels_desc_host, int n_levels, int channels, int batch_size,
                                       const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h,
                                       int pooled_w, int pooled_z, int sampling_ratio, int feats_bf16,
                                       const void *grad_output_bf16, float *accum_f32, void *d_feats_all_bf16_or_null,
                                       int64_t total_rows, void *stream);

/* ---- RPN loss (csrc/rpn_loss.hip): RPNLossComputation.__call__ (modeling/rpn/loss_3d.py:201-251), one objectness group.
 * Per example the BalancedPositiveNegativeSampler (modeling/balanced_positive_negative_sampler.py:19-68):
 *   num_pos = min(P, num_pos_max), num_neg = min(N, batch_size_per_image - num_pos), num_pos_max = int(B * f);
 * then, over the batch's N_s = sum of num_pos + num_neg sampled anchors,
 *   box_loss = sum over sampled positives and 7 components of smoothL1(|pred - target|) / N_s,
 *              smoothL1(d) = 0.5 d^2 / beta if d < beta else d - 0.5 beta  (layers/smooth_l1_loss.py:34-52, 'Diff'),
 *   obj_loss = sum over sampled anchors of max(x,0) - x y + log1p(exp(-|x|)) / N_s  (y = 1 positive, 0 negative).
 * N_s == 0 gives NaN for both (0 / 0, the reference's mean of nothing) and zero gradients.
 *
 * Labels: matched indices as aabr_rpn_label_generation writes them, >= 0 positive, -1 negative, -2 ignored.
 * Index mapping (nothing concatenated): anchor (example b, map m, row r of b's sites in m, yaw a) is
 *   objectness / regression element (site_begin[b][m] + r) * A + a of map m ([V_m * A] / [V_m * A, 7], the grid's row order),
 *   label / regression-target element seg_begin[b][m] + r * A + a of example b's lists (label_ptrs[b] int64 [N_b],
 *   target_ptrs[b] fp32 [N_b, 7]),
 * with seg_begin_host [nb][n_maps + 1] / site_begin_host [nb][n_maps] the tables aabr_rpn_label_generation_targets takes.
 *
 * Selection rule.  fmix32 = murmur3's 32-bit finaliser (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35;
 * h ^= h >> 16).  Anchor key: h = fmix32(seed ^ 0x9E3779B9), then h = fmix32(h ^ v) for v in (example, map, x, y, z, a)
 * in that order, x y z = the site's coordinates (columns 0..2 of the map's coords), example = index in the call.  The
 * sample of a class is its k anchors with the smallest (key, map, x, y, z, a), compared lexicographically: a uniform
 * random subset per seed, the same anchors whatever the grid's row order.
 *
 * Outputs: selected int64 [nb][batch_size_per_image] = indices into the concatenation of the examples' label lists
 * (example-major), positives then negatives, each in selection order, -1 padded; info int32 [nb][8] = num_pos, num_neg,
 * P, N, candidates pos / neg, overflow (never set for a list of < 2^31 hashed keys unless > 1024 - B keys share the
 * 24-bit prefix at the cut; the sample is then not exact), N_s of the batch; obj_loss / box_loss one fp32 each.
 * Inputs fp32 (input_bf16 = 0) or bf16 (1), every map alike; arithmetic fp32.  1 <= batch_size_per_image <= 512.
 * Launches: 1 memset + 4 per chunk of 16 examples + 1; sums in fixed order (no float atomics): bit-identical run to run.
 * scratch: aabr_rpn_loss_scratch_words(nb) int32, 8-byte aligned.                                                     */
int64_t aabr_rpn_loss_scratch_words(int nb);
int aabr_rpn_loss_forward(int n_maps, const void *const *coords_ptrs, const void *const *obj_ptrs,
                          const void *const *reg_ptrs, int input_bf16, int num_anchors, int nb,
                          const int32_t *seg_begin_host, const int32_t *site_begin_host, const void *const *label_ptrs,
                          const void *const *target_ptrs, uint32_t seed, int batch_size_per_image, int num_pos_max,
                          float beta, int64_t *selected, int32_t *info, float *obj_loss, float *box_loss,
                          int32_t *scratch, void *stream);
/* Gradients of the two losses: the caller zeroes grad_obj_ptrs[m] / grad_reg_ptrs[m] (input dtype, the maps' shapes);
 * one launch per chunk of 16 examples writes (sigmoid(x) - y) / N_s * g_obj at every sampled anchor and
 * smoothL1'(d) sign(pred - target) / N_s * g_box at every sampled positive.  g_obj / g_box: device fp32 scalars (the
 * upstream gradients); selected / info: the forward's.                                                                */
int aabr_rpn_loss_backward(int n_maps, const void *const *obj_ptrs, const void *const *reg_ptrs, int input_bf16,
                           int num_anchors, int nb, const int32_t *seg_begin_host, const int32_t *site_begin_host,
                           const void *const *target_ptrs, int batch_size_per_image, float beta,
                           const int64_t *selected, const int32_t *info, const float *grad_obj_loss,
                           const float *grad_box_loss, void *const *grad_obj_ptrs, void *const *grad_reg_ptrs,
                           void *stream);
/* The loss with separated-classifier groups (the reference's loop over the groups, seperate_classifier.py:68-109, as ONE
 * call): segment e = b G + g (scene b, group g) is to these calls what an example is to aabr_rpn_loss_forward.
 *   seg_begin_host / site_begin_host stay per SCENE ([nb][...]), shared by a scene's G segments.
 *   obj_ptrs[m] / reg_ptrs[m] point at the GROUP-MAJOR allocations aabr_rpn_head_grouped_forward writes ([G][V_m, A] and
 *   [G][V_m, A, 7]), rows_host[m] = V_m: a head value of segment e sits g V_m A behind the plain index.
 *   label_ptrs[e] / target_ptrs[e] are per segment (the labels of the scene's anchors against group g's ground truth).
 *   The key hashes the SCENE index b, not e: one grouped call selects exactly what G plain calls (one per group, over the
 *   nb scenes) with the same seed select, and gives the same bits.
 * Outputs: selected [nb G][B], indices into the concatenation of the label lists of the segment's GROUP, scene-major (what
 *   the plain call on that group returns); info [nb G][8], word 7 = N_s of the segment's group over the batch;
 *   obj_loss [G], box_loss [G]: each group's sums in scene order / its N_s (NaN for an empty group sample, zero
 *   gradients).  Any nb G, chunked by 16 segments; 2 <= G <= 16.
 * Launches: forward 1 memset + 4 per chunk + 1; backward 1 per chunk, upstream gradients grad_obj_loss [G],
 * grad_box_loss [G], the gradient allocations group-major like the inputs and zeroed by the caller.
 * scratch: aabr_rpn_loss_grouped_scratch_words(nb, G) int32, 8-byte aligned (0 for an unsupported shape).              */
int64_t aabr_rpn_loss_grouped_scratch_words(int nb, int G);
int aabr_rpn_loss_grouped_forward(int n_maps, const void *const *coords_ptrs, const void *const *obj_ptrs,
                                  const void *const *reg_ptrs, const int64_t *rows_host, int input_bf16, int num_anchors,
                                  int nb, int G, const int32_t *seg_begin_host, const int32_t *site_begin_host,
                                  const void *const *label_ptrs, const void *const *target_ptrs, uint32_t seed,
                                  int batch_size_per_image, int num_pos_max, float beta, int64_t *selected,
                                  int32_t *info, float *obj_loss, float *box_loss, int32_t *scratch, void *stream);
int aabr_rpn_loss_grouped_backward(int n_maps, const void *const *obj_ptrs, const void *const *reg_ptrs,
                                   const int64_t *rows_host, int input_bf16, int num_anchors, int nb, int G,
                                   const int32_t *seg_begin_host, const int32_t *site_begin_host,
                                   const void *const *target_ptrs, int batch_size_per_image, float beta,
                                   const int64_t *selected, const int32_t *info, const float *grad_obj_loss,
                                   const float *grad_box_loss, void *const *grad_obj_ptrs, void *const *grad_reg_ptrs,
                                   void *stream);
/* List form of the sampler (BalancedPositiveNegativeSampler.__call__): label_ptrs[b] int64 [n_host[b]] with >= 1 positive,
 * 0 negative, anything else ignored.  Same kernels and rule with key h = fmix32(seed ^ 0x9E3779B9), h = fmix32(h ^ v) for
 * v in (example, index), ties by index.  selected / info as above (indices into the concatenated lists; info[7] = 0);
 * pos_masks[b] / neg_masks[b] (optional, uint8 [n_host[b]], zeroed by the caller) get a 1 at every selected entry.
 * scratch: aabr_rpn_loss_scratch_words(nb).                                                                            */
int aabr_sample_list(int nb, const void *const *label_ptrs, const int64_t *n_host, uint32_t seed,
                     int batch_size_per_image, int num_pos_max, int64_t *selected, int32_t *info,
                     void *const *pos_masks, void *const *neg_masks, int32_t *scratch, void *stream);
/* smooth_l1_loss (layers/smooth_l1_loss.py:34-52, yaw mode 'Diff': the same term on all 7 columns) on n elements:
 * out = sum smoothL1(|input - target|) / divisor (n for size_average, 1 for the sum), fixed-order reduction;
 * backward: grad_input = smoothL1'(d) sign(input - target) * grad_out / divisor.  input fp32 / bf16, target fp32.
 * scratch: aabr_smooth_l1_scratch_floats() fp32.                                                                      */
int64_t aabr_smooth_l1_scratch_floats(void);
int aabr_smooth_l1_forward(const void *input, const float *target, int64_t n, int input_bf16, float beta, float divisor,
                           float *out, float *scratch, void *stream);
int aabr_smooth_l1_backward(const void *input, const float *target, int64_t n, int input_bf16, float beta, float divisor,
                            const float *grad_out, void *grad_input, void *stream);

/* ---- ROI box post-processor (csrc/roi_post.hip): PostProcessor.forward of the box head
 * (modeling/roi_heads/box_head_3d/inference.py:44-162) for a batch of nb scenes in five launches, no host read.
 * Inputs: class_logits fp32 [N, C] (class 0 = background), box_regression fp32 [N, 7 C] (class_specific != 0) or [N, 7]
 * (one box per row, shared by its classes, inference.py:102-104), proposals fp32 [N, 7] yx_zb; the scenes' rows are
 * concatenated scene-major, n_host[nb] rows each, N their sum.
 *   prob = softmax(class_logits, -1) (:57); boxes = BoxCoder3D.decode (box_coder_3d.py:53-80: weights_host[7], clip) --
 *   the arithmetic of aabr_box_decode; per scene and class j = 1 .. C-1 (:125-141): the rows with prob[:, j] >
 *   score_thresh (strict), their boxes clamped for the NMS only (sizes 3:5 >= nms_min_yx, size 5 >= nms_min_z,
 *   structures/boxlist_ops_3d.py:42-44), the pre_max best in descending score, greedy suppression by the rule of
 *   aabr_rotate_nms_sorted (its own mask and scan code), the first post_max survivors; per scene the classes in
 *   ascending order, each in survivor order; if there are M > detections_per_img = D > 0 of them, those with score >=
 *   the D-th largest stay, in place (:153-161: ties at the cut all stay); D <= 0 keeps all.
 * Equal scores are ordered by ascending proposal row, in the list and at the pre_max cut (torch.topk leaves that open).
 * Outputs: prob [N, C] and boxes [N, C, 7] (each optional: NULL keeps it in scratch); per scene b at the fixed stride
 * cap = (C - 1) * post_max: det_rows int64 (scene-local proposal row), det_labels int64, det_scores fp32, det_boxes
 * [., 7] (the unclamped boxes); info int32 [nb][8] = detections kept, detections before the cut, candidates over all
 * classes, largest candidate count of a class, largest survivor count of a class, 0, 0, 0.
 * Limits: 2 <= C <= 32, 1 <= nb <= 16, 1 <= post_max <= pre_max <= 2048, N * C * 7 < 2^31.  A scene with no row, a class
 * without a candidate and N = 0 are legal (empty lists).  Bit-identical run to run (no float atomics).
 * scratch: aabr_roi_post_scratch_words(nb, largest n_host, C, pre_max) int32 words (-1: bad shape), 8-byte aligned.   */
int64_t aabr_roi_post_scratch_words(int nb, int64_t n_max, int C, int pre_max);
int aabr_roi_post_detections(const float *class_logits, const float *box_regression, const float *proposals, int nb,
                             const int64_t *n_host, int C, int class_specific, const float *weights_host, float clip,
                             float score_thresh, float nms_thresh, float nms_min_yx, float nms_min_z, int only_xy,
                             int pre_max, int post_max, int detections_per_img, float *prob, float *boxes,
                             int64_t *det_rows, int64_t *det_labels, float *det_scores, float *det_boxes, int32_t *info,
                             int32_t *scratch, void *stream);
/* The same with the coder's form as an argument: corner_coder = 0 is aabr_roi_post_detections itself; 1 decodes with
 * BoxCoder3D(is_corner_roi=True).decode, the arithmetic of aabr_box_decode_corner (box_regression then holds two-corner
 * encodings, proposals stay yx_zb and so do the decoded boxes).  Softmax, NMS, the per-scene cut and the five launches
 * are the same code. */
int aabr_roi_post_detections_coder(const float *class_logits, const float *box_regression, const float *proposals, int nb,
                                   const int64_t *n_host, int C, int class_specific, const float *weights_host,
                                   int corner_coder, float clip, float score_thresh, float nms_thresh, float nms_min_yx,
                                   float nms_min_z, int only_xy, int pre_max, int post_max, int detections_per_img,
                                   float *prob, float *boxes, int64_t *det_rows, int64_t *det_labels, float *det_scores,
                                   float *det_boxes, int32_t *info, int32_t *scratch, void *stream);

/* ---- Box-head loss (csrc/roi_loss.hip): FastRCNNLossComputation of the box head
 * (modeling/roi_heads/box_head_3d/loss.py:137-382, the non-separated path) in two stages, `subsample` and `__call__`.
 *
 * Stage 1, aabr_roi_targets: proposals of a batch -> per-proposal match, label and regression target -> the balanced
 * sample, for nb scenes with no host read.  proposals fp32 [N, 7] yx_zb and targets fp32 [G, 7] / target_labels int64 [G]
 * are scene-major, n_host[b] / g_host[b] rows per scene.  Per proposal of scene b (one pass; the [G_b, n_b] matrix is
 * stored only when iou_out is given):
 *   IoU with every ground-truth box of the scene = boxlist_iou_3d(target, proposal, aug_thickness, criterion), the
 *   arithmetic of aabr_boxes_iou_3d (aug_host[4] = {target_Y, target_Z, anchor_Y, anchor_Z}; loss.py:164 passes
 *   criterion -1); the scene's boxes are staged in LDS in chunks of 128, so G_b is unbounded;
 *   Matcher(fg_iou, bg_iou, allow_low_quality_matches=False), yaw_diff=None (loss.py:578-582, matcher.py:58-106):
 *   matched_val = the maximum over the ground truths, matched_idx = its scene-local index (the first maximum at ties,
 *   the rule of aabr_rpn_label_generation), -1 where matched_val < bg_iou, -2 where bg_iou <= matched_val < fg_iou;
 *   a NaN entry (0 / 0 in the z factor: only_xy off, two zero heights at the same z, no thickness clamp) is the
 *   maximum of its proposal, the first one by index, as in torch.max: matched_val is NaN and, both comparisons being
 *   false, the proposal is matched to that box;
 *   labels (loss.py:213-222) = target_labels[matched_idx] for a match, 0 for -1, -1 for -2;
 *   regression_targets (loss.py:225-227) = BoxCoder3D.encode(target[max(matched_idx, 0)], proposal) for EVERY proposal,
 *   bit-equal to aabr_box_encode on the same rows (weights_host[7]).
 * A scene with G_b == 0 (loss.py:200-206): labels 0, regression targets 0, matched_idx -1, matched_val 0.  A scene with
 * n_b == 0 is legal here and yields an empty sample (the reference's Matcher raises "No proposal boxes available").
 * Then BalancedPositiveNegativeSampler over `labels` per scene -- the kernels and the rule of aabr_sample_list (key over
 * (seed, scene, scene-local row); >= 1 positive, 0 negative, everything else ignored; csrc/sample_shared.h is compiled
 * into both files) -- and the compaction of loss.py:279-281 (nonzero(pos | neg)): the sampled rows in ASCENDING
 * proposal row, not in selection order.
 * Outputs over all N proposals: matched_idx int64, matched_val fp32, labels int64, regression_targets fp32 [N, 7];
 * iou_out (optional, may be NULL): the unmasked [G_b, n_b] matrices back to back.  Per scene at the fixed stride B =
 * batch_size_per_image: samp_rows int64 (scene-local proposal rows, -1 padded), samp_labels int64 (-1 padded),
 * samp_targets fp32 [., 7] and samp_boxes fp32 [., 7] (the proposals' rows; 0 padded); info int32 [nb][8] = sampled
 * count, num_pos, num_neg, P, N, ignored, the sampler's overflow flag (see aabr_rpn_loss_forward), 0.
 * Limits: 1 <= nb <= 16, 1 <= batch_size_per_image <= 512 (the sampler's), 0 <= num_pos_max <= batch_size_per_image,
 * N < 2^31.  Launches: 1 memset + 6 kernels (match, the sampler's 4, compaction), whatever nb, G and the class count.
 * No float atomics: bit-identical run to run.  scratch: aabr_roi_targets_scratch_words(nb) int32, 8-byte aligned.       */
int64_t aabr_roi_targets_scratch_words(int nb);
int aabr_roi_targets(const float *proposals, const float *targets, const int64_t *target_labels, int nb,
                     const int64_t *n_host, const int64_t *g_host, const float *aug_host, int criterion, int only_xy,
                     float fg_iou, float bg_iou, const float *weights_host, uint32_t seed, int batch_size_per_image,
                     int num_pos_max, int64_t *matched_idx, float *matched_val, int64_t *labels,
                     float *regression_targets, float *iou_out, int64_t *samp_rows, int64_t *samp_labels,
                     float *samp_targets, float *samp_boxes, int32_t *info, int32_t *scratch, void *stream);
/* The same with the coder's form as an argument: corner_coder = 0 is aabr_roi_targets itself; 1 makes the regression
 * targets BoxCoder3D(is_corner_roi=True).encode(target[max(matched_idx, 0)], proposal), bit-equal to
 * aabr_box_encode_corner on the same rows.  Matching, labels, the sampler, the compaction and the launch count (1 memset
 * + 6 kernels) do not depend on it. */
int aabr_roi_targets_coder(const float *proposals, const float *targets, const int64_t *target_labels, int nb,
                           const int64_t *n_host, const int64_t *g_host, const float *aug_host, int criterion,
                           int only_xy, float fg_iou, float bg_iou, const float *weights_host, int corner_coder,
                           uint32_t seed, int batch_size_per_image, int num_pos_max, int64_t *matched_idx,
                           float *matched_val, int64_t *labels, float *regression_targets, float *iou_out,
                           int64_t *samp_rows, int64_t *samp_labels, float *samp_targets, float *samp_boxes,
                           int32_t *info, int32_t *scratch, void *stream);
/* Stage 2 (loss.py:295-382): class_logits [n, C], box_regression [n, 7 C] (class_specific != 0) or [n, 7], both fp32
 * (input_bf16 = 0) or bf16 (1), arithmetic fp32; labels int64 [n]; regression_targets fp32 [n, 7]; beta > 0 (the
 * reference: 1 / 5).
 *   cls_loss = sum over the n rows of (logsumexp(x) - x[label]) / n                      (F.cross_entropy, mean)
 *   box_loss = sum over the rows with label > 0 and 7 columns of smoothL1(|pred - target|) / n   (loss.py:369-377:
 *              labels.numel(), not the positive count); pred = columns 7 label .. 7 label + 6 when class specific,
 *              0 .. 6 otherwise; smoothL1 as in aabr_rpn_loss_forward.
 * Per-row terms are added per thread in row order, per workgroup in a fixed tree, then in workgroup order: bit-identical
 * run to run.  n == 0 gives NaN for both (0 / 0) and there is no gradient to write.  A label outside [0, C) reads nothing
 * out of bounds: the row adds nothing to either loss, gets zero gradients, and *flag (int32) becomes 1 (0 otherwise).
 * Launches: 2.  scratch: aabr_roi_box_loss_scratch_floats() fp32.
 * Backward (1 launch) writes EVERY element of grad_logits [n, C] and grad_regression (the input's shape and dtype; no
 * fill by the caller): (softmax(x) - onehot(label)) * g_cls / n, and smoothL1'(d) sign(pred - target) * g_box / n in
 * the seven columns of a row with label > 0, exact zeros everywhere else.  g_cls / g_box: device fp32 scalars.       */
int64_t aabr_roi_box_loss_scratch_floats(void);
int aabr_roi_box_loss_forward(const void *class_logits, const void *box_regression, int input_bf16, int64_t n, int C,
                              int class_specific, const int64_t *labels, const float *regression_targets, float beta,
                              float *cls_loss, float *box_loss, int32_t *flag, float *scratch, void *stream);
int aabr_roi_box_loss_backward(const void *class_logits, const void *box_regression, int input_bf16, int64_t n, int C,
                               int class_specific, const int64_t *labels, const float *regression_targets, float beta,
                               const float *grad_cls_loss, const float *grad_box_loss, void *grad_logits,
                               void *grad_regression, void *stream);

/* ---- the box head with separated-classifier groups (MODEL.SEPARATE_CLASSES; the reference's
 * modeling/seperate_classifier.py, which loops over the groups around its single-group code).  Added after 640 without a
 * bump: symbols only.  G groups share the C_tot = num_input_classes + G - 1 columns of class_logits.  The description is
 * two host tables -- class_nums int32 [G] and cols int32 [sum of class_nums], the groups' column lists one after the
 * other, each in group-local order with the group's background column first -- and travels to the kernels by value: no
 * device table.  Every non-background column index is that class's original label.  Validated before any HIP call
 * (AABR_EINVAL): 2 <= G <= 8, 2 <= C_tot <= 32, every group 1 .. C_tot columns, every column index in [0, C_tot) and in
 * at most one group; besides the limits of the plain entry points.  Box regression is class agnostic ([n, 7]).
 *
 * Stage 1 (SeperateClassifier.seperate_subsample): a proposal takes part only in its own group's ground truth.  The
 * proposals are concatenated scene-major and group-major inside a scene; segment s = scene G + group has n_host[s] rows
 * (host-known) and is to aabr_roi_targets_grouped what a scene is to aabr_roi_targets_coder: IoU with the ground truth of
 * its scene whose label lies in its group, the Matcher, the label as the GROUP-LOCAL id (0 background, -1 ignored), the
 * coder's encode, the balanced sampler per segment (hash key over (seed, s, segment-local row)) and the ascending
 * compaction; samp_* and info are [nb G][...].  A segment without ground truth of its group: all background, zero
 * targets.  The host never learns how many boxes of a scene fall into a group:
 *   aabr_roi_gt_group_keys (1 launch): target_labels int64 (the batch's ground truth, scene-major, g_host[b] rows for
 *     scene b, ORIGINAL labels) -> keys int64: (b G + g) 32 + i when the label is column cols[g][i], nb G 32 (behind
 *     every segment) when no group owns it;
 *   the caller sorts the keys ascending and STABLY and passes the sorted keys and the permutation (gt_perm[k] = the
 *     batch row at sorted position k): a segment's ground truth is then one run in the order (group-local label, row),
 *     the order in which the reference concatenates a group's targets, so the first maximum of a tie is the lower
 *     group-local label and then the lower row;
 *   aabr_roi_targets_grouped (1 memset + 6 launches whatever nb and G) finds each segment's run by binary search on the
 *     device and reads targets [sum g_host, 7] through gt_perm.  matched_idx is the row in the scene's own list.
 * nb G <= 16 segments.  scratch: aabr_roi_targets_scratch_words(nb G).  The IoU matrices are not stored.               */
int aabr_roi_gt_group_keys(const int64_t *target_labels, int nb, const int64_t *g_host, int G, int C_tot,
                           const int32_t *class_nums_host, const int32_t *cols_host, int64_t *keys, void *stream);
int aabr_roi_targets_grouped(const float *proposals, const float *targets, const int64_t *gt_keys, const int64_t *gt_perm,
                             int nb, int G, const int64_t *n_host, const int64_t *g_host, const float *aug_host,
                             int criterion, int only_xy, float fg_iou, float bg_iou, const float *weights_host,
                             int corner_coder, uint32_t seed, int batch_size_per_image, int num_pos_max,
                             int64_t *matched_idx, float *matched_val, int64_t *labels, float *regression_targets,
                             int64_t *samp_rows, int64_t *samp_labels, float *samp_targets, float *samp_boxes,
                             int32_t *info, int32_t *scratch, void *stream);
/* Stage 2 (roi_cross_entropy_seperated, roi_box_loss_seperated): class_logits [n, C_tot], box_regression [n, 7] (fp32 or
 * bf16), per row sep_id int32 (its group), labels int64 (group-local) and regression_targets fp32 [n, 7]:
 *   cls_loss[g] = sum over the rows of group g of (logsumexp over the group's columns - x[cols[g][label]]) / n_g
 *   box_loss[g] = sum over the group's rows with label > 0 and 7 columns of smoothL1(|pred - target|) / n_g
 * n_g, the group's row count, is counted on the device and left in group_rows int32 [G] for the backward; n_g = 0 gives
 * NaN for that group only.  Sums in a fixed order (per thread in row order, a fixed tree per workgroup, then workgroup
 * order), no float atomics.  A sep_id outside [0, G) (the row is in no group) or a label outside [0, class_nums[g]) (the
 * row counts in n_g) is never used as an index: the row adds nothing, gets zero gradients, *flag becomes 1.  Launches: 2.
 * scratch: aabr_roi_box_loss_grouped_scratch_floats() fp32.  Backward (1 launch): g_cls / g_box are device fp32 [G];
 * EVERY element of grad_logits [n, C_tot] and grad_regression [n, 7] is written, exact zeros outside the row's group. */
int64_t aabr_roi_box_loss_grouped_scratch_floats(void);
int aabr_roi_box_loss_grouped_forward(const void *class_logits, const void *box_regression, int input_bf16, int64_t n,
                                      int G, int C_tot, const int32_t *class_nums_host, const int32_t *cols_host,
                                      const int32_t *sep_id, const int64_t *labels, const float *regression_targets,
                                      float beta, float *cls_loss, float *box_loss, int32_t *group_rows, int32_t *flag,
                                      float *scratch, void *stream);
int aabr_roi_box_loss_grouped_backward(const void *class_logits, const void *box_regression, int input_bf16, int64_t n,
                                       int G, int C_tot, const int32_t *class_nums_host, const int32_t *cols_host,
                                       const int32_t *sep_id, const int64_t *labels, const float *regression_targets,
                                       float beta, const int32_t *group_rows, const float *grad_cls_loss,
                                       const float *grad_box_loss, void *grad_logits, void *grad_regression,
                                       void *stream);
/* ---- the corner-connection losses of the corner-ROI box head (csrc/corner_loss.hip; the reference's `*_corsem.yaml`
 * configurations: geometric_pull_loss, semantic_pull_loss, semantic_push_loss, MODEL.LOSS.WEIGHTS[4:7]).  Added after 640
 * without a bump: symbols only.
 *
 * Label side, aabr_corner_tables (3 launches whatever nb; no host read), run behind aabr_roi_targets_coder on its outputs.
 * targets [sum g_host, 7] yx_zb, matched_idx int64 [sum n_host] (>= 0: the scene-local ground-truth row), samp_rows int64
 * [nb][B] (ascending scene-local proposal rows, -1 behind the sample), samp_boxes fp32 [nb][B][7], B =
 * batch_size_per_image <= 512, nb <= 16.  Outputs, every element written:
 *   tg_xyz fp32 [2 G, 3]      the two top corners of every ground-truth box, moved towards their midpoint by half the
 *                             thickness (bounding_box_3d.py:270-291) -- corner 2 g + c of the batch's box g;
 *   tg_connect int32 [2 G, 3] per ground-truth corner the first three OTHER corners of its scene, in ascending scene-local
 *                             corner index, closer than 0.1; -1 where there are fewer (bounding_box_3d.py:451-477);
 *   pos_pos int64 [nb][B]     the scene's positives -- sampled rows with matched_idx >= 0 -- ordered by (matched target,
 *                             position in the sample): the position of the k-th; -1 behind the p_b positives;
 *   connect_ids int32 [nb][2 B][8]  per proposal corner 2 k + c: over its own ground-truth corner and that corner's up to
 *                             three connected ones, the corners 2 k' + c' of the first four positives k' of each one's box
 *                             (c' = that ground-truth corner's parity) -- 16 slots, sorted descending, cut to 8, -1 where
 *                             there are fewer (box_head_3d/loss.py:22-99); rows behind 2 p_b are -1;
 *   corner_xyz fp32 [nb][2 B][3]    the proposal corners' coordinates, as tg_xyz of the sampled boxes; zeros behind 2 p_b;
 *   info int32 [nb][8]        [0] = p_b, [1] = g_host[b], the rest 0.
 *
 * Loss (box_head_3d/loss.py:384-499).  corners_semantic fp32 [n, 16] over the concatenated samples: scene b owns m_host[b]
 * rows (their sum is n), p_host[b] <= 512 of them positives, described by the device arrays pos_pos_ptrs[b] (int64
 * [p_b]), ids_ptrs[b] (int32 [2 p_b, 8]) and xyz_ptrs[b] (fp32 [2 p_b, 3]) -- host arrays of nb device pointers, e.g. rows
 * of the padded outputs above.  Corner 2 k + c of scene b has the semantic vector corners_semantic[row of the k-th
 * positive][8 c .. 8 c + 7].  Per scene, with N = 2 p_b corners, C_i = {i} + the entries of i's table row:
 *   geometric pull = sum over table entries e of i with |xyz_e - xyz_i| < 0.2 of that distance / max(their count - N, 1)
 *   semantic pull  = sum over i and a in C_i of |sem_a - sem_i| / max(sum |C_i| - N, 1)
 *   semantic push  = sum over i and a not in C_i with |xyz_a - xyz_i| < 0.5 of max(1 - |sem_a - sem_i|, 0) /
 *                    max(their count, 1)
 * and each loss is the sum over the scenes / nb; a scene without positives adds 0.  losses fp32 [3] = geometric pull,
 * semantic pull, semantic push; counts int32 [nb][4] = the three counts in that order and N, kept for the backward.  fp32
 * sums in a fixed order (per tile of aabr_corner_loss_tile() corners, per thread, a fixed tree per workgroup, workgroup
 * order, scene order), integer counts, no float atomics: bit-identical run to run.  Table entries outside [0, N) and
 * positions outside [0, m_b) are never used as an index.  Launches: 2.  scratch: aabr_corner_loss_scratch_words(nb) int32.
 * Backward (1 launch): grad_pull_loss / grad_push_loss are device fp32 scalars (the geometric loss depends on the
 * proposals only: no gradient); EVERY element of grad_corners_semantic [n, 16] is written, exact zeros in the rows that
 * are no positive; the gradient of a distance that is exactly 0 is 0.                                               */
int aabr_corner_loss_tile(void);
int64_t aabr_corner_loss_scratch_words(int nb);
int aabr_corner_tables(const float *targets, int nb, const int64_t *n_host, const int64_t *g_host,
                       const int64_t *matched_idx, const int64_t *samp_rows, const float *samp_boxes,
                       int batch_size_per_image, float *tg_xyz, int32_t *tg_connect, int64_t *pos_pos,
                       int32_t *connect_ids, float *corner_xyz, int32_t *info, void *stream);
int aabr_corner_loss_forward(const float *corners_semantic, int64_t n, int nb, const int64_t *m_host,
                             const int64_t *p_host, const void *const *pos_pos_ptrs, const void *const *ids_ptrs,
                             const void *const *xyz_ptrs, float *losses, int32_t *counts, int32_t *scratch, void *stream);
int aabr_corner_loss_backward(const float *corners_semantic, int64_t n, int nb, const int64_t *m_host,
                              const int64_t *p_host, const void *const *pos_pos_ptrs, const void *const *ids_ptrs,
                              const void *const *xyz_ptrs, const int32_t *counts, const float *grad_pull_loss,
                              const float *grad_push_loss, float *grad_corners_semantic, void *stream);
/* Detections (SeperateClassifier.post_processor): aabr_roi_post_detections_coder with groups.  sep_id int32 [N], rows in
 * any order inside a scene.  Per row the softmax over its group's columns (group-local order), every other column of
 * prob an exact 0; boxes [N, 7].  Per (scene, foreground column c): the rows OF c's GROUP with prob > score_thresh
 * (membership is tested; a zero is not relied on), then the same NMS.  Per scene the groups ascending, each group's
 * columns in group-local order, the detections_per_img cut PER (scene, group) with ties at the cut staying; the label is
 * the column index (the original label); capacity (C_tot - G) post_max rows per scene.  A sep_id outside [0, G): the
 * row is no candidate and info[b][5] becomes 1.  5 launches; scratch: aabr_roi_post_scratch_words(nb, n_max, C_tot,
 * pre_max).                                                                                                          */
int aabr_roi_post_detections_grouped(const float *class_logits, const float *box_regression, const float *proposals,
                                     const int32_t *sep_id, int nb, const int64_t *n_host, int G, int C_tot,
                                     const int32_t *class_nums_host, const int32_t *cols_host, const float *weights_host,
                                     int corner_coder, float clip, float score_thresh, float nms_thresh, float nms_min_yx,
                                     float nms_min_z, int only_xy, int pre_max, int post_max, int detections_per_img,
                                     float *prob, float *boxes, int64_t *det_rows, int64_t *det_labels, float *det_scores,
                                     float *det_boxes, int32_t *info, int32_t *scratch, void *stream);

/* ---- the box head's dense layers (csrc/roi_mlp.hip): FPN2MLPFeatureExtractor after its pooler
 * (roi_box_feature_extractors.py:46-169: Conv3d([1,1,pz]) + BatchNorm3d + ReLU, fc6 + ReLU, fc7 + ReLU) and FPNPredictor
 * (roi_box_predictors.py:34-109) as a dense fp32 GEMM family on v_mfma_f32_32x32x2_f32 (fp32 storage, the pooled operand
 * also in bf16 through the _pooled_bf16 entry points below; exact fp32:
 * every result element is an fmaf chain over its reduction).  A layer is Y [M, N] = act(A W^T + bias) with W [N, K]
 * row-major, the reference's parameter layout (nn.Linear.weight; Conv3d.weight viewed as [R, C pz]).
 *   shapes: any M >= 0 (M == 0 launches no kernel and succeeds; the weight gradient of M == 0 is a memset to zero), any
 *   N >= 1, K >= 4 with K % 4 == 0, all below 2^31 - 256; anything else, a null pointer or a negative size: AABR_EINVAL.
 *   a_layout: AABR_MLP_ROWS = A is row-major [M, K] (hw, pz ignored); AABR_MLP_POOLED = A is the pooler's
 *   [n, C, hw, pz] tensor read in place: row m = n hw + s, column k = c pz + z, element ((n C + c) hw + s) pz + z
 *   (M % hw == 0, K % pz == 0) -- no transposed copy of the activation is written in either direction.
 * aabr_roi_mlp_forward:         Y = A W^T (+ bias if not NULL) (ReLU if relu).                          1 launch.
 * aabr_roi_mlp_backward_input:  dA [M, K] = (dY . mask) W, mask = (Y > 0) read with dY when Y is not NULL (the forward
 *   applied ReLU), all ones when Y is NULL; dA is stored in a_layout (pooled: what aabr_roi_pool_backward reads), every
 *   element exactly once.                                                                                1 launch.
 * aabr_roi_mlp_backward_weight: dW [N, K] = (dY . mask)^T A and, when db is not NULL, db [N] = column sums of dY . mask
 *   (added in row order inside the same kernel).  Deterministic, no float atomics: when aabr_roi_mlp_dw_splits(M, N, K)
 *   > 1 the reduction over M is cut into that many runs of whole 32-row chunks, one workgroup per run and tile, each
 *   writing its partial to scratch (fp32 [aabr_roi_mlp_dw_scratch_floats(M, N, K)], may be NULL when that is 0), and a
 *   second launch adds the partials in run order.  perm_hw > 0 (K % perm_hw == 0, R = K / perm_hw): A's column
 *   k' = s R + r is stored at dW column r perm_hw + s -- fc6's gradient in the reference's layout while the GEMM ran on
 *   the packed weight.                                                                         1 launch, 2 when split.
 * aabr_roi_mlp_pack_fc6: Wp [N, hw R] with Wp[o, s R + r] = W[o, r hw + s]: fc6.weight (columns in x.view(N, -1) order
 *   over the reference's [N, R, h, w] activation) for the activation kept as rows [N hw, R].            1 launch.
 * Dispatch (host functions, so tests can place shapes on both sides):
 *   aabr_roi_mlp_tile(rows, cols): edge of the square output tile a workgroup owns, for an output of [rows, cols]:
 *     128 when there are at least 192 tiles of 128 x 128, else 64 (0 for an empty output).  Forward: (M, N); input
 *     gradient: (M, K); weight gradient: (N, K).  The reduction runs in chunks of 32.
 *   aabr_roi_mlp_dw_splits(M, N, K): runs the weight gradient's reduction is cut into: min(512 / tiles, 64,
 *     ceil(M / 256)), at least 1, then rounded so every run is whole 32-row chunks and none is empty.
 * BatchNorm3d + ReLU between the convolution and fc6 is aabr_bn_forward / aabr_bn_backward over the [n hw, R] rows
 * (leakiness 0); the statistics are NOT taken from the GEMM's write-out.
 * Launch counts of the whole head, whatever the ROI count (roi_glue.box_head_mlp + box_predictions).  Library launches:
 * forward 7 = conv GEMM 1 + BatchNorm 2 + fc6 pack 1 + fc6 1 + fc7 1 + predictor 1 (both linears as one GEMM); backward
 * 10 to 14 = per GEMM 1 input gradient + 1 weight gradient (+ 1 when split: 13 at the default sizes, where all but
 * fc6's are) + BatchNorm's own 2.  On top of these, torch's own small kernels in the Python layer: forward 2 copies
 * (torch.cat of the predictor's two weights and two biases) and 1 add when the BatchNorm tracks running statistics
 * (num_batches_tracked); backward 5 for the two column views of the predictor's result (two zero fills, two copies, one
 * add), besides the gradient accumulation into the parameters that every autograd function has.                     */
#define AABR_MLP_ROWS 0
#define AABR_MLP_POOLED 1
int aabr_roi_mlp_tile(int64_t rows, int64_t cols);
int aabr_roi_mlp_dw_splits(int64_t M, int64_t N, int64_t K);
int64_t aabr_roi_mlp_dw_scratch_floats(int64_t M, int64_t N, int64_t K);
int aabr_roi_mlp_forward(const float *A, int a_layout, int64_t hw, int pz, const float *W, const float *bias, int relu,
                         int64_t M, int64_t N, int64_t K, float *Y, void *stream);
int aabr_roi_mlp_backward_input(const float *dY, const float *Y, const float *W, int64_t M, int64_t N, int64_t K,
                                int a_layout, int64_t hw, int pz, float *dA, void *stream);
int aabr_roi_mlp_backward_weight(const float *dY, const float *Y, const float *A, int a_layout, int64_t hw, int pz,
                                 int64_t M, int64_t N, int64_t K, int64_t perm_hw, float *dW, float *db, float *scratch,
                                 void *stream);
int aabr_roi_mlp_pack_fc6(const float *W, int64_t N, int64_t R, int64_t hw, float *Wp, void *stream);
/* The pooled operand in bf16 storage, read and written in place: each mirrors its namesake above with a_layout fixed to
 * AABR_MLP_POOLED.  A_bf16 / dA_bf16 are the pooler's [n, C, hw, pz] tensor in bf16 (aabr_roi_pool_*_pooled_bf16), 4-byte
 * aligned; an element is widened on load (exact), the LDS image, the MFMA chain, the mask, the bias and the ReLU are the
 * fp32 form's, so Y, dW and db are bit for bit what the fp32 form gives on the widened tensor, and dA_bf16 is ONE rounding
 * (nearest even) of the fp32 form's dA, every element written once.  dY, Y, W, dW, db and scratch stay fp32.  Tile,
 * splits, scratch size, launch counts and shape checks are those of the fp32 forms at the same (M, N, K).            */
int aabr_roi_mlp_forward_pooled_bf16(const void *A_bf16, int64_t hw, int pz, const float *W, const float *bias, int relu,
                                     int64_t M, int64_t N, int64_t K, float *Y, void *stream);
int aabr_roi_mlp_backward_input_pooled_bf16(const float *dY, const float *Y, const float *W, int64_t M, int64_t N,
                                            int64_t K, int64_t hw, int pz, void *dA_bf16, void *stream);
int aabr_roi_mlp_backward_weight_pooled_bf16(const float *dY, const float *Y, const void *A_bf16, int64_t hw, int pz,
                                             int64_t M, int64_t N, int64_t K, int64_t perm_hw, float *dW, float *db,
                                             float *scratch, void *stream);
/* fc6 over WINDOWS of the convolution rows: the corner form of the box head (MODEL.CORNER_ROI,
 * roi_box_feature_extractors.py:122-147).  X is the convolution + BatchNorm result kept as rows [n_rois ph pw, R]; the
 * extractor cuts the pw (= 11) axis into cor0 = w 0..2, body = w 2..8, cor1 = w 8..10 and runs an fc6 on each part made
 * contiguous.  Here a window [w0, w0 + wlen) is a third operand layout of the same GEMM template, read and written in
 * place: row m of the operand is ROI n's window, column k = (h wlen + wl) R + r is X[(n ph + h) pw + w0 + wl][r], so
 * K = ph wlen R and the packed weight is aabr_roi_mlp_pack_fc6 with hw = ph wlen.  `blocks` = 2 stacks two windows that
 * share a weight into one GEMM with M = 2 n_rois: rows 0 .. n_rois - 1 use w0[0], rows n_rois .. 2 n_rois - 1 use w0[1]
 * on ROI m - n_rois (the two corners: w0 = {0, 8}).  Limits: ph, pw, R, wlen >= 1, 0 <= w0, w0 + wlen <= pw, K % 4 == 0,
 * ph pw R and M below 2^31 - 256; otherwise AABR_EINVAL.  Tile and split decisions are those of the dense entry points
 * at the same (M, N, K).
 * aabr_roi_mlp_forward_window:         Y [M, N] = act(Xwin W^T + bias).                                 1 launch.
 * aabr_roi_mlp_backward_weight_window: dW, db and scratch as aabr_roi_mlp_backward_weight.     1 launch, 2 when split.
 * aabr_roi_mlp_backward_input_window:  (dY . mask) W stored into the windows of dX in place.  acc_w0 / acc_w1: absolute
 *   w positions (or -1) at which the value is ADDED to what dX holds instead of stored -- the windows of the head overlap
 *   at w = 2 and w = 8.  The order that makes dX complete without a zero fill and without atomics: the body GEMM
 *   (w0 = 2, wlen = 7, acc -1, -1) first, then on the same stream the corner GEMM (w0 = {0, 8}, wlen = 3, acc 2, 8), which
 *   stores w 0, 1, 9, 10 and adds into w 2 and 8; each element is touched by one thread per launch, so two runs give the
 *   same bits.  The windows of a two-block call may not overlap each other.                              1 launch. */
typedef struct AabrMlpWindow {
  int64_t n_rois;
  int32_t ph, pw, R;           /* the convolution rows are [n_rois ph pw, R]                                          */
  int32_t wlen;                /* window length along the pw axis                                                     */
  int32_t blocks;              /* 1 or 2 row blocks of n_rois rows each                                               */
  int32_t w0[2];               /* first w of each block's window (w0[1] ignored when blocks == 1)                     */
} AabrMlpWindow;
int aabr_roi_mlp_forward_window(const float *X, const AabrMlpWindow *win, const float *W, const float *bias, int relu,
                                int64_t N, float *Y, void *stream);
int aabr_roi_mlp_backward_input_window(const float *dY, const float *Y, const float *W, const AabrMlpWindow *win,
                                       int64_t N, int acc_w0, int acc_w1, float *dX, void *stream);
int aabr_roi_mlp_backward_weight_window(const float *dY, const float *Y, const float *X, const AabrMlpWindow *win,
                                        int64_t N, int64_t perm_hw, float *dW, float *db, float *scratch, void *stream);

/* ---- the RPN head (csrc/rpn_head.hip): SingleConvRPNHead_Sparse3D (modeling/rpn/rpn_sparse3d.py:81-131) over the rows
 * of every feature map in one launch, on v_mfma_f32_32x32x2_f32 (every element an exact fmaf chain); the feature rows
 * in fp32 storage, or in bf16 through the _bf16 entry points below:
 *   t = relu(f W1^T + b1),  obj = t Wc^T + bc,  reg = t Wr^T + br
 * with f [rows, C] the rows of a map and W1 [C, C], Wc [A, C], Wr [7 A, C] the Conv2d weights viewed as [out, in].
 * Output channel order is the reference's permute + reshape ('box_toghter'): objectness [rows, A], box_regression
 * [rows, A, 7] with channel a 7 + j -- the [site, yaw] flatten order aabr_rpn_decode_maps, aabr_rpn_label_generation and
 * aabr_rpn_loss_forward read.
 *   shapes: 1 <= n_maps <= 8; C in {32, 64, 96, 128}; 1 <= A <= 4; any rows >= 0 (a map with 0 rows contributes
 *   nothing and its pointers are not read).  Anything else, a null pointer or a negative size: AABR_EINVAL.
 * maps_host: a host array of n_maps records (read during the call, passed to the kernels by value; nothing is
 *   concatenated).  `hidden`: one fp32 [sum of rows, C] allocation, map-major, or NULL.
 * aabr_rpn_head_forward: a workgroup owns aabr_rpn_head_tile_rows(C) consecutive rows of one map, forms t in LDS and
 *   both outputs from it; t is stored to `hidden` only when that is not NULL (evaluation: it never reaches memory; the
 *   outputs are the same bits either way).  1 launch, whatever n_maps; none when every map is empty.
 * aabr_rpn_head_backward: the records' objectness / box_regression point at d_obj / d_reg (read only; NULL = zeros),
 *   d_features receives d_f (every element stored exactly once).  dW1 [C, C], db1 [C], dWc [A, C], dbc [A],
 *   dWr [7 A, C], dbr [7 A] are overwritten.  Deterministic, no float atomics: tile i of the concatenated tile list goes
 *   to workgroup i mod G, G = aabr_rpn_head_groups(total_tiles); ONE fused kernel forms dt = (d_out [Wc; Wr]) . (t > 0),
 *   stores d_f = dt W1 and keeps its share of all six sums in registers; each workgroup writes one partial to
 *   `scratch` (fp32 [aabr_rpn_head_scratch_floats(total_tiles, C, A)]) and a second launch adds the partials in
 *   workgroup order.  2 launches (main, reduce; no weight pack is needed), whatever n_maps.  Every map empty: no
 *   launch, the six gradients are set to zero (memsets).
 * Host functions of the shape only (never of the device), so tests can place shapes on both sides:
 *   aabr_rpn_head_tile_rows(C): 64 for a supported C, else 0.  total_tiles = sum over maps of ceil(rows / tile_rows).
 *   aabr_rpn_head_groups(total_tiles): min(total_tiles, 256); 0 for total_tiles < 1.
 *   aabr_rpn_head_scratch_floats(total_tiles, C, A): groups * (C C + 32 C + C + 32); 0 for an unsupported shape.      */
/* The _bf16 entry points read `features` and write `d_features` as bf16 rows [rows, C] through the same two pointers
 * (both 4-byte aligned); every other field, and the record's 40 bytes, are the same.                                  */
typedef struct AabrRpnMap {
  const float *features;       /* [rows, C] fp32 feature rows of the map                                              */
  int64_t rows;
  float *objectness;           /* forward: output [rows, A]; backward: d_obj (read only) or NULL                      */
  float *box_regression;       /* forward: output [rows, A, 7]; backward: d_reg (read only) or NULL                   */
  float *d_features;           /* backward: output [rows, C]; unused by forward                                       */
} AabrRpnMap;
int aabr_rpn_head_tile_rows(int C);
int aabr_rpn_head_groups(int64_t total_tiles);
int64_t aabr_rpn_head_scratch_floats(int64_t total_tiles, int C, int A);
int aabr_rpn_head_forward(const AabrRpnMap *maps_host, int n_maps, int C, int A, const float *W1, const float *b1,
                          const float *Wc, const float *bc, const float *Wr, const float *br, float *hidden, void *stream);
int aabr_rpn_head_backward(const AabrRpnMap *maps_host, int n_maps, int C, int A, const float *W1, const float *Wc,
                           const float *Wr, const float *hidden, float *dW1, float *db1, float *dWc, float *dbc,
                           float *dWr, float *dbr, float *scratch, void *stream);
/* The head with separated-classifier groups (MODEL.SEPARATE_CLASSES with SEPARATE_RPN, rpn_sparse3d.py:95-131), G =
 * len(SEPARATE_CLASSES) + 1 RPN branches on one hidden layer.  The weights come in the reference's layout, so its
 * state_dict loads unchanged: Wc [A G, C] with row a G + g, Wr [7 A G, C] with row a 7 G + 7 g + k; bc [A G], br [7 A G].
 * The outputs are written GROUP-MAJOR: a record's objectness points at [G][rows, A] and box_regression at
 * [G][rows, A, 7] (d_obj / d_reg of the backward call likewise), so group g's slice is a contiguous tensor in the plain
 * [site, yaw] layout above; the permutation is done in the forward write-out and in the backward's load of d_out, no
 * tensor is permuted or copied.  hidden and d_features as in the plain calls.
 *   shapes: as above, and 2 <= G <= 8, A G <= 16 (up to 128 output columns, four MFMA tiles); else AABR_EINVAL.
 * The reduction order over the hidden units is aabr_rpn_head_forward's: `hidden`, and group g's objectness and
 * box_regression, are bit for bit what aabr_rpn_head_forward gives with rows a G + g of Wc and a 7 G + 7 g + k of Wr.
 * Launches as in the plain calls: forward 1; backward 2, partials in `scratch`
 * (fp32 [aabr_rpn_head_grouped_scratch_floats(total_tiles, C, A, G)] = groups * (C C + NP C + C + NP), NP = 8 A G rounded
 * up to a multiple of 32; 0 for an unsupported shape) added in workgroup order; every map empty: no launch, memsets. */
int64_t aabr_rpn_head_grouped_scratch_floats(int64_t total_tiles, int C, int A, int G);
int aabr_rpn_head_grouped_forward(const AabrRpnMap *maps_host, int n_maps, int C, int A, int G, const float *W1,
                                  const float *b1, const float *Wc, const float *bc, const float *Wr, const float *br,
                                  float *hidden, void *stream);
int aabr_rpn_head_grouped_backward(const AabrRpnMap *maps_host, int n_maps, int C, int A, int G, const float *W1,
                                   const float *Wc, const float *Wr, const float *hidden, float *dW1, float *db1,
                                   float *dWc, float *dbc, float *dWr, float *dbr, float *scratch, void *stream);
/* bf16 feature storage (rpn_sparse3d.py:81-131 as above; each mirrors the fp32 entry point of the same name, same
 * arguments, shapes, scratch and launches).  AabrRpnMap.features / .d_features point at bf16 rows, 4-byte aligned.  The
 * rows are widened (exact) into the fp32 kernel's own LDS images, so objectness, box_regression, `hidden` and the six
 * weight gradients -- all fp32 -- are bit for bit the fp32 entry point's on the widened rows.  d_features is the one
 * output in bf16: each fp32 value the fp32 entry point would store is rounded once (nearest even), every element stored
 * exactly once.                                                                                                       */
int aabr_rpn_head_forward_bf16(const AabrRpnMap *maps_host, int n_maps, int C, int A, const float *W1, const float *b1,
                               const float *Wc, const float *bc, const float *Wr, const float *br, float *hidden,
                               void *stream);
int aabr_rpn_head_backward_bf16(const AabrRpnMap *maps_host, int n_maps, int C, int A, const float *W1, const float *Wc,
                                const float *Wr, const float *hidden, float *dW1, float *db1, float *dWc, float *dbc,
                                float *dWr, float *dbr, float *scratch, void *stream);
int aabr_rpn_head_grouped_forward_bf16(const AabrRpnMap *maps_host, int n_maps, int C, int A, int G, const float *W1,
                                       const float *b1, const float *Wc, const float *bc, const float *Wr,
                                       const float *br, float *hidden, void *stream);
int aabr_rpn_head_grouped_backward_bf16(const AabrRpnMap *maps_host, int n_maps, int C, int A, int G, const float *W1,
                                        const float *Wc, const float *Wr, const float *hidden, float *dW1, float *db1,
                                        float *dWc, float *dbc, float *dWr, float *dbr, float *scratch, void *stream);

/* ---- the optimizer step (csrc/solver.hip, csrc/solver_segs.h): torch.optim.SGD with momentum and weight decay
 * (dampening 0, no Nesterov form) over all parameters of one flat fp32 buffer in ONE launch.  Per element, fp32, each
 * operation rounded on its own, in this order:
 *   g  = widen(grad);  g = g * grad_scale  only when grad_scale != 1
 *   d  = g + wd * p                        only when wd != 0 (else d = g)
 *   m' = momentum * m + d                  only when momentum != 0 (else momentum_buf is neither read nor written)
 *   p' = p - lr * m'
 * A parameter is a segment (flat offset, numel, group) of `flat`; a group is one (lr, weight_decay) pair, at most 8.
 * aabr_sgd_chunk_elems(): the most elements of a chunk.  Segments are cut into chunks of at most that many elements;
 *   every cut inside a segment lies on a multiple of 4 elements of the flat offset; a segment of 0 elements has no chunk.
 * aabr_sgd_chunk_table: host only.  Cuts the segments (ascending, non-overlapping, inside [0, n)) and writes one record
 *   of 4 int64 words per chunk -- flat offset, the segment's flat offset, elements, segment index * 8 + group -- to
 *   table_host [cap_chunks][4]; table_host NULL: counts only.  Returns the number of chunks, or -1 (aabr_last_error).
 *   The caller uploads the table once and keeps the host copy.
 * aabr_sgd_momentum_step: min(n_chunks, 2048) workgroups of 256 threads grid-stride over chunk_table (device).  flat and
 *   momentum_buf: fp32 [n], 16-byte aligned, the same layout.  Exactly one gradient source:
 *     grad_flat       a device buffer [n] of the flat layout, fp32 or (grad_is_bf16 = 1) bf16, read in place;
 *     grad_ptr_table  a device table [n_segs] of 64-bit gradient addresses, one contiguous gradient per segment; a
 *                     segment whose address is 0 is skipped (p and m stay bit for bit).
 *   A gradient whose address does not allow 4-element loads at a chunk is read element by element; p and m are always
 *   accessed 16 bytes at a time between a segment's first and last multiple of 4.
 *   lr, wd: host arrays of n_groups values, passed to the kernel by value (a new learning rate is no device write).
 *   chunk_table_host: the host copy of the uploaded table; its last record is checked against n and n_segs.
 *   Refused with AABR_EINVAL before any launch: both gradient sources or neither, n_groups outside 1 .. 8, a null
 *   pointer, a negative size, a misaligned buffer, a table whose last chunk ends past n.  n_chunks == 0: no launch.   */
int aabr_sgd_chunk_elems(void);
int64_t aabr_sgd_chunk_table(const int64_t *seg_off, const int64_t *seg_numel, const int32_t *seg_group, int64_t n_segs,
                             int64_t n, int64_t *table_host, int64_t cap_chunks);
int aabr_sgd_momentum_step(float *flat, float *momentum_buf, int64_t n, const int64_t *chunk_table,
                           const int64_t *chunk_table_host, int64_t n_chunks, int64_t n_segs, const void *grad_flat,
                           const void *grad_ptr_table, int grad_is_bf16, const float *lr, const float *wd, int n_groups,
                           float momentum, float grad_scale, void *stream);

/* ---- detection evaluation (csrc/det_eval.hip, csrc/det_eval.h): eval_detection_suncg of the reference
 * (data3d/evaluation/suncg/suncg_eval.py:733-986, use_07_metric=True; the other value is not implemented) for a whole
 * data set, in two entries with the caller's sort between them.  4 library launches + that sort for a whole evaluation,
 * whatever the number of scenes, classes and boxes; no host read inside; no float atomics: bit-identical run to run.
 *
 * Inputs are scene-major concatenations over n_scenes >= 1 scenes (<= 65535): det_boxes fp32 [n_det, 7] yx_zb,
 * det_labels int64, det_scores fp32; gt_boxes fp32 [n_gt, 7], gt_labels int64.  det_begin / gt_begin: DEVICE int64
 * arrays of n_scenes + 1 ascending row offsets (first 0, last n_det / n_gt), which the caller forms from list lengths it
 * knows on the host; offsets that disagree with the totals are clamped to them.  n_det_max: the largest scene's detection
 * count (it sizes the grid).  C: classes, background included, 2 <= C <= 32.
 *
 * aabr_det_eval_match (3 launches; 1 without ground truth or without detections).  Per detection of scene s, label l:
 *   IoU with every ground-truth box of the scene whose label is l = boxlist_iou_3d(gt, pred, aug, criterion=-1,
 *   flag='eval'), the arithmetic of aabr_boxes_iou_3d (aug_host[4] = {target_Y, target_Z, anchor_Y, anchor_Z}, ground
 *   truth on the target side; only_xy != 0: no z factor, what the reference's DEBUG = 1 forces);
 *   pred_iou = the maximum, gt_index = the first maximum's index AMONG THE SCENE'S BOXES OF CLASS l (a NaN entry wins,
 *   the first NaN by index, as np.argmax / np.max: the order of aabr_roi_targets); gt_index = -1 where
 *   pred_iou < iou_thresh (strict: IoU == iou_thresh matches, a NaN matches); no box of the class in the scene:
 *   gt_index = -1, pred_iou = 0;
 *   match = 1 for the first detection in score order among those of the scene that share a gt_index >= 0 and label, 0
 *   for every other detection.  Score order: descending score (-0.0 == +0.0, NaN scores behind -inf), equal scores by
 *   ascending detection row.  Implemented as an integer 64-bit minimum over (score key, row), not a sequential loop;
 *   sort_key int64 [n_det] = (label << 32) | score key, ascending = class-major, descending score.
 *   A detection label outside [0, C) is skipped (gt_index -1, pred_iou 0, match 0, sort_key of class C: behind every
 *   class) and a ground-truth label outside [0, C) matches nothing; both are counted in aabr_det_eval_curves' cls.
 *   iou_out (optional, NULL): fp32 matrices [g_s, n_s] back to back at iou_begin[s] (DEVICE int64 [n_scenes]); only the
 *   entries of equal label are written.  scratch: aabr_det_eval_scratch_words(n_det, n_gt) int32, 8-byte aligned.
 * The caller then sorts sort_key ascending with a STABLE sort: sorted_key and `order` (the source row of each position).
 * aabr_det_eval_curves (1 launch, one workgroup per class, which walks the class's run serially on one CU; a class's
 * detection count is bounded only by n_det < 2^31 -- addressing, not speed: nothing above a few thousand per class is timed):
 *   over class l's run of the sorted order, tp = cumsum(match == 1), fp = cumsum(match == 0) as integers,
 *   rec = tp / n_pos[l], prec = tp / (tp + fp) in float64 (0 / 0 = NaN for a class without ground truth);
 *   rows fp64 [n_det, 4] = rec, prec, score, pred_iou at every sorted position (rows of skipped labels: not written);
 *   cls [C][64] 64-bit words per class: doubles 0 = 11-point AP (p / 11 added over t = 0.0 + 0.1 i, i = 0 .. 10),
 *   1 .. 44 = the 11 rows [t, max nan_to_num(prec) over rec >= t else 0, min score over rec <= t else max score + 0.01,
 *   max nan_to_num(pred_iou) over rec >= t else 0], 45 .. 46 / 47 .. 48 = prec, rec at k = count(score > 0.5 / 0.7) - 1
 *   (k = -1: the last position); all NaN for a class without a detection; int64 56 = n_pos, 57 = detections, 58 = tp
 *   total, 59 = first sorted position; in class 0's row 60 / 61 = ground-truth / detection labels outside [0, C).
 *   aabr_det_eval_scan_chunk(): detections per pass of the scan (the results do not depend on it).
 * Refused with AABR_EINVAL before any launch: C outside 2 .. 32, n_scenes outside 1 .. 65535, a negative count, 2^31 or
 * more rows, n_det_max > n_det, a null pointer, a misaligned scratch.                                                  */
int64_t aabr_det_eval_scratch_words(int64_t n_det, int64_t n_gt);
int aabr_det_eval_match(const float *det_boxes, const int64_t *det_labels, const float *det_scores,
                        const float *gt_boxes, const int64_t *gt_labels, int64_t n_scenes, const int64_t *det_begin,
                        const int64_t *gt_begin, int64_t n_det, int64_t n_gt, int64_t n_det_max, int C, float iou_thresh,
                        const float *aug_host, int only_xy, int64_t *gt_index, float *pred_iou, int8_t *match,
                        int64_t *sort_key, float *iou_out, const int64_t *iou_begin, int32_t *scratch, void *stream);
int aabr_det_eval_curves(const int64_t *sorted_key, const int64_t *order, const int8_t *match, const float *pred_iou,
                         const float *det_scores, const int64_t *gt_labels, int64_t n_det, int64_t n_gt, int C,
                         double *rows, int64_t *cls, void *stream);
int aabr_det_eval_scan_chunk(void);

/* ---- sparse pooling (csrc/pool.hip): MaxPooling, AveragePooling and UnPooling of the reference (SCN/CPU/MaxPooling.cpp,
 * AveragePooling.cpp, UnPooling.cpp), forward and backward, each pass ONE gather launch over one table of a strided rule
 * book (table int32 [vol][rows]: the source row per destination row and filter offset, -1 where absent).  No atomics, no
 * memset, no host read: every destination element is written once, bit-identical run to run.
 *
 * aabr_pool_gather:  dst[r, dst_col0 + c] = reduce over o = 0 .. vol-1 ascending, for table[o][r] >= 0, of
 *   x = src[table[o][r] * src_stride + col0 + c], c in [0, planes):
 *   mode 0 (MAX0)  acc = +0.0f; if (acc < x) acc = x      -> max(0, inputs), a NaN input is ignored
 *   mode 1 (SUM)   acc = +0.0f; acc += x / div            (div > 0: one correctly rounded fp32 division per term);
 *                  div == 0: acc += x                      (no division at all)
 *   The columns of dst rows outside [dst_col0, dst_col0 + planes) up to dst_width are written 0.
 *   MaxPooling / AveragePooling forward: the book's `out` table (div = vol for the average); AveragePooling backward: its
 *   `inn` table, div = vol; UnPooling forward: `inn` of the book (fine, coarse, size, stride), div = 0; its backward: `out`.
 * aabr_pool_max_backward (over the book's `inn` table, rows_in input rows):
 *   dx[r, col0 + c] = sum over o ascending, for orow = table_in[o][r] >= 0, of
 *                     (y[orow, c] == x[r, col0 + c]) ? dy[orow, c] : 0     (+0.0 == -0.0; a NaN never matches)
 *   x and dx [rows_in, x_stride] with x_stride == col0 + planes, y and dy [*, planes]; dx[:, 0 .. col0) = 0.
 * bf16 != 0: every feature pointer holds bf16 (widened to fp32, the same fp32 operations, one round-to-nearest-even at
 * the store; the comparison is on the stored values); else fp32.  16-byte accesses when planes, column offsets and row
 * strides are multiples of 4 (fp32) / 8 (bf16) and the bases are 16-byte aligned, one element per lane otherwise.
 * Zero destination rows: AABR_OK without a launch.  Refused with AABR_EINVAL before any launch: planes <= 0, vol <= 0, an
 * unknown mode, div < 0, a negative row count, columns outside their row, a null pointer with rows > 0.                 */
int aabr_pool_gather(const void *src, int bf16, int64_t src_stride, int col0, int planes, const int32_t *table, int vol,
                     int64_t rows_dst, int mode, float div, void *dst, int64_t dst_stride, int dst_col0, int dst_width,
                     void *stream);
int aabr_pool_max_backward(const void *x, const void *y, const void *dy, int bf16, int64_t x_stride, int col0, int planes,
                           const int32_t *table_in, int vol, int64_t rows_in, void *dx, void *stream);

/* ---- merging wall detections by their corners (csrc/merge_corners.hip, csrc/merge_corners.h): merge_by_corners /
 * merge_walls_by_corners of the reference (maskrcnn_benchmark/structures/bounding_box_3d.py:843-923) for every scene of
 * a call in ONE launch, one workgroup per scene; no host read; no atomics: bit-identical run to run.
 *
 * boxes fp32 [n, 7] yx_zb, scene-major; labels int64 [n] (NULL: every row is a wall); scene_begin: DEVICE int64 array of
 * n_scenes + 1 ascending row offsets (first 0, last n), formed by the caller from list lengths it knows on the host;
 * max_scene_rows: the largest scene's row count (host).  The rows of a scene with labels == wall_label are its walls, in
 * ascending row order; wall w has corners 2w and 2w+1.
 *   1. per wall yxzb_to_2corners and corners_top_offseted: the two top corners pulled in by half the thickness;
 *   2. for i = 0 .. 2W-1 on the corners as the earlier steps left them: S = every corner closer to corner i than
 *      `threshold` (distance sqrt(fma(dz,dz,fma(dy,dy,dx*dx))), strict <), without the other corner of i's wall; a wall
 *      with both corners in S skips the step; otherwise, with |S| > 1, every corner of S takes the mean of S (summed in
 *      ascending corner index from 0, one fp32 addition at a time, one division by |S|) and is flagged merged;
 *   3. per wall both corners are pushed outward from their midpoint by half the thickness; x0 y0 x1 y1 from the pushed
 *      corners, z1 = the mean of their z, z0 of EVERY wall = the scene's mean z0 (summed in ascending wall order),
 *      corners_to_yxzb.  A wall whose corners end at one point divides by zero and gives the IEEE result.
 * boxes_out fp32 [n, 7] (not boxes itself): the walls rebuilt, every other row copied bit for bit.  merged (optional, NULL)
 * int32 [n, 2]: 1 where a wall's corner 0 / 1 was merged, 0 elsewhere and for rows that are no wall.  W = 1 runs 1 and 3.
 * aabr_merge_corners_max_walls(): the walls per scene the kernel's LDS image is built for (2048).  A scene's wall count is
 * known on the device only, so its ROW count is held to that limit: max_scene_rows beyond it is refused, never truncated.
 * Refused with AABR_EINVAL before any launch: that, a negative count, 2^28 or more rows, max_scene_rows > n, rows without
 * a scene, a null pointer with rows > 0, boxes_out == boxes.  n_scenes == 0: AABR_OK without a launch.                   */
int aabr_merge_corners_max_walls(void);
int aabr_merge_walls_by_corners(const float *boxes, const int64_t *labels, int64_t n, const int64_t *scene_begin,
                                int64_t n_scenes, int64_t max_scene_rows, int64_t wall_label, float threshold,
                                float *boxes_out, int32_t *merged, void *stream);

#ifdef __cplusplus
}
#endif
#endif
