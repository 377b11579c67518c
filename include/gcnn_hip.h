/* gcnn_hip.h -- C ABI of libgcnn_hip.so: the MI355X (gfx950) implementation of the bipartite GCNN hot path of
 * stefanvanberkum/gcnn-cut-selector.
 *
 * The reference has no native layer and no FFI: its hot path is Python calling TensorFlow ops
 * (/root/reference/model.py).  Each entry point below therefore cites the reference *Python* interface whose
 * arithmetic it replaces.  All pointers are DEVICE pointers unless marked "host"; all matrices are row-major fp32,
 * indices int32; `stream` is a hipStream_t passed as void*.  Every function returns 0 on success, a negative
 * GCNN_E_* code on bad arguments and a positive hipError_t on a HIP failure; no function allocates device memory
 * (workspaces are passed in), synchronises the device or throws.  A *_layout_for or *_fill_table that returns a GCNN_E_* code has
 * written nothing: the caller's struct or table is as it was.
 */
#ifndef GCNN_HIP_H
#define GCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCNN_EMB 64
#define GCNN_N_PARAMS 62          /* arrays in a checkpoint, model.py:53-56 */
#define GCNN_E_BADARG (-1)
#define GCNN_E_WORKSPACE (-2)
#define GCNN_E_UNSUPPORTED (-4)   /* sizes outside what a specialised entry point handles: use the general path */
#define GCNN_E_HIP (-3)           /* a HIP call failed inside an entry point whose return value is a count */

/* ---- parameter layout --------------------------------------------------------------------------------------
 * All 62 model variables live in ONE flat fp32 buffer, in the reference's checkpoint order
 * (model.py:53-56, 215; shapes model.py:174-208, 486-508), each tensor starting at a multiple of 4 floats.
 * Gradients and Adam moments use the same layout. */
int gcnn_abi_version(void);
int gcnn_param_count(void);                                   /* 62 */
int gcnn_param_total_floats(void);                            /* size of the flat buffer */
int gcnn_param_info(int index, int* offset, int* rows, int* cols, int* trainable);

/* ---- per-launch timing (a measuring aid; bench.py's roofline_step) ------------------------------------------------
 * Between gcnn_profile_begin() and gcnn_profile_end() every kernel launch the library makes is bracketed by two HIP events
 * on its stream.  gcnn_profile_end waits for those events (the ONE entry point that synchronises), stores up to `capacity`
 * kernel names (static strings) and durations in milliseconds, launch by launch, and returns the number of launches seen
 * (possibly > capacity; at most 512 are recorded), or GCNN_E_HIP.  Single-threaded use only, one session at a time, all launches of
 * a session on streams of the device that was current at gcnn_profile_begin (events are per device). */
int gcnn_profile_begin(void);
int gcnn_profile_end(int32_t capacity, const char** names /* host, optional */, float* ms /* host, optional */);

/* ---- sizes ------------------------------------------------------------------------------------------------ */
typedef struct gcnn_dims {
    int32_t n_cons, n_vars, n_cuts;        /* TOTAL node counts of the stacked batch (model.py:273-275) */
    int32_t n_cons_edges, n_cut_edges;     /* E1, E2 */
} gcnn_dims;

/* One edge set in both receiver orders (built by gcnn_graph_build): by-left CSR and by-variable CSR. */
typedef struct gcnn_graph {
    const int32_t* l_ptr;   /* [n_left+1]  segment offsets, edges grouped by left (constraint/cut) node */
    const int32_t* l_oth;   /* [E]         variable index of each edge, by-left order */
    const float*   l_coef;  /* [E]         raw edge feature, by-left order */
    const int32_t* v_ptr;   /* [n_var+1]   segment offsets, edges grouped by variable node */
    const int32_t* v_oth;   /* [E]         left index of each edge, by-variable order */
    const float*   v_coef;  /* [E]         raw edge feature, by-variable order */
    int32_t l_max_deg;      /* longest by-left segment, 0 = unknown.  Edge passes give segments that are long for the list's */
    int32_t v_max_deg;      /* longest by-variable segment, 0 = unknown.  mean degree a wave of their own in an extra launch,
                               which is skipped when the list is known to hold none. */
} gcnn_graph;

/* ---- graph plan: COO -> receiver-sorted CSR in both orders -------------------------------------------------
 * Replaces nothing arithmetic in the reference; it is the index structure that lets tf.scatter_nd
 * (model.py:568-569) and the gradients of tf.gather (model.py:564-565) run as atomic-free segmented sums.
 * edge_inds is the reference's [2,E] int32 tensor (row 0 = left id, row 1 = variable id, utils.py:110,234);
 * any edge order is accepted (stable sort => deterministic summation order). */
size_t gcnn_graph_temp_bytes(int32_t n_edges);
/* one pass over the list: flags[0] != 0 <=> some index is out of range; flags[1] != 0 <=> NOT sorted by left id */
int gcnn_graph_check(const int32_t* edge_inds, int32_t n_edges, int32_t n_left, int32_t n_var, int32_t* flags,
                     void* stream);
/* left_sorted != 0 (as established by gcnn_graph_check; the reference's get_state emits (row, col)-sorted lists,
 * utils.py:102-104) skips the by-left sort: the by-left order is then the input order. */
int gcnn_graph_build(const int32_t* edge_inds, const float* edge_feats, int32_t n_edges, int32_t n_left,
                     int32_t n_var, int32_t left_sorted, int32_t* l_ptr, int32_t* l_oth, float* l_coef, int32_t* v_ptr, int32_t* v_oth,
                     float* v_coef, int32_t* l_perm /* optional [E]: by-left position -> input edge id */, void* temp,
                     size_t temp_bytes, void* stream);

/* ---- device-side batch collation: utils.load_batch's stacking (utils.py:389-426) on a device-resident sample store
 * The store keeps every sample's arrays (features, targets and both CSR orders of both edge sets) concatenated in
 * HBM with SAMPLE-LOCAL index values.  Because a mini-batch is a disjoint union, its arrays are the chosen samples'
 * segments laid end to end with indices shifted by the sample's position in the batch (utils.py:401-407) -- CSR
 * included, so no sort runs per batch.  One launch performs all copies.  A job copies `width` 4-byte words per unit
 * (node row / edge / cut); units of sample-slot s go from src unit src_off[unit_kind][s].. to dst unit
 * dst_off[unit_kind][s]..; int32 arrays add dst_off[add_kind][s] (add_kind < 0: plain copy); is_ptr arrays
 * (segment offsets, width 1) get one trailing entry = dst_off[add_kind][batch].
 * jobs: HOST array (<= 24); src_off [n_kinds][batch] and dst_off [n_kinds][batch+1]: DEVICE int64;
 * max_words: the largest job's output size in words (sizes the grid). */
typedef struct gcnn_collate_job {
    const void* src;
    void* dst;
    int32_t unit_kind, width, add_kind, is_ptr;
} gcnn_collate_job;
int gcnn_collate(const gcnn_collate_job* jobs, int32_t n_jobs, const int64_t* src_off, const int64_t* dst_off,
                 int32_t batch, int64_t max_words, void* stream);

/* ---- standalone scatter-sum pass (K9): tf.scatter_nd(updates=[E,64], indices, shape=[R,64]), model.py:568-569
 * seg_ptr[R+1] are receiver-sorted segment offsets; perm (optional) maps sorted position -> row of `msg`
 * (NULL when msg is already receiver-sorted).  out[r] = sum of the segment's rows, 0 for empty segments. */
int gcnn_seg_sum_f32(const float* msg, const int32_t* seg_ptr, const int32_t* perm, int32_t n_recv, float* out,
                     void* stream);
/* its transpose (the gradient of the pass): d_msg[perm[i]] = d_out[recv(i)] */
int gcnn_seg_bcast_f32(const float* d_out, const int32_t* seg_ptr, const int32_t* perm, int32_t n_recv,
                       float* d_msg, void* stream);

/* ---- node GEMMs on the fp32 MFMA: Keras Dense(64) layers, model.py:174-208, 486-508 ---------------------------
 * forward:  y = act( (sa*xa) @ wa [+ xb @ wb] [+ bias] [+ deg (x) bd] ),  deg_r = seg_ptr[r+1]-seg_ptr[r]
 *           (the deg term is the hoisted bias of feature_module_final, model.py:499-500 summed by :568).
 *           xa, xb, y: [n,64]; wa, wb: [64,64] Keras (in,out) layout; sa: optional device scalar.
 * backward: dy <- dy * (ymask > 0) in place when ymask != NULL, then
 *           dx (=|+=) so * (dy @ wa^T)  and optionally  dx2 (=|+=) dy @ wb^T   (beta 0 = overwrite, 1 = accumulate) */
int gcnn_linear_fwd(const float* xa, const float* sa, const float* wa, const float* xb, const float* wb,
                    const float* bias, const float* bd, const int32_t* seg_ptr, int32_t relu, float* y, int32_t n,
                    void* stream);
int gcnn_linear_bwd(float* dy, const float* ymask, const float* wa, const float* so, float* dx, int32_t beta,
                    const float* wb, float* dx2, int32_t beta2, int32_t n, void* stream);

/* ---- fused edge pass of PartialGraphConvolution.call, model.py:563-569, with Dense(feature_module_final) hoisted --
 * forward:  s_out[r] = sum_{e in seg(r)} relu(s1 * (PL[l_e] + c_e*w_edge + PR[v_e])),  c_e = (coef_e+e_shift)*e_scale
 *           p_recv = projected table of the receiving side [n_recv,64] (constraint/cut side when from_v=True,
 *           model.py:553-556), p_oth = the other side's table, gathered by oth[e].
 *           Optional output for the backward pass: n_rows [n_recv,64] = number of active edges ([s1*J_e > 0]) per
 *           receiver and channel.  Nothing is stored per edge.  Tables hold at most 2^24 rows (gathers use 32-bit byte offsets).
 * bwd_recv: element-wise, because d_s[r] is constant over a segment: d_p_recv = s1*d_s*n_rows.
 * bwd_send: segments grouped by the SENDING node u; the ReLU pattern is recomputed from the two projected tables with the
 *           forward's own expression (bit-identical): with r = oth[e], J_e = (c_e*w_edge + p_send[u]) + p_recv[r] and
 *           t_e = [s1*J_e > 0] * d_s[r]:
 *           d_p_send[u] = s1*sum_{e in seg(u)} t_e ;  the gradient of feature_module_edge's kernel (model.py:490-492),
 *           s1*sum_e c_e*t_e, is left as *n_parts partial rows dw_partial[i][64] (one per thread block, fixed summation
 *           order; the caller adds the rows up): the main blocks' rows first, then, when the pass ran them (max_degree
 *           0 or beyond the long-segment threshold), one per long-segment block.  dw_partial must hold GCNN_EDGE_DW_PARTS
 *           rows. */
#define GCNN_EDGE_DW_PARTS 16384
int gcnn_conv_edge_fwd(const int32_t* seg_ptr, const int32_t* oth, const float* coef, int32_t n_recv, int32_t n_edges,
                       const float* p_recv, const float* p_oth, const float* w_edge, const float* e_shift,
                       const float* e_scale, const float* s1, float* s_out, float* n_rows /* optional */,
                       int32_t max_degree /* longest segment, 0 = unknown */, void* stream);
int gcnn_conv_edge_bwd_recv(const float* d_s, const float* n_rows, const float* s1, int32_t n_recv, float* d_p_recv,
                            void* stream);
int gcnn_conv_edge_bwd_send(const int32_t* seg_ptr, const int32_t* oth, const float* coef, int32_t n_send, int32_t n_edges,
                            const float* p_send, const float* p_recv, const float* w_edge, const float* e_shift,
                            const float* e_scale, const float* s1, const float* d_s, float* d_p_send, float* dw_partial,
                            int32_t* n_parts /* host */, int32_t max_degree /* longest segment, 0 = unknown */, void* stream);

/* ---- whole-model forward: GCNN.call, model.py:257-300 ------------------------------------------------------
 * params: flat buffer (layout above).  cons/var/cut feats: [C,4], [V,14], [K,6] raw features (PreNorm applied
 * inside, model.py:365-382).  workspace: gcnn_workspace_floats(dims) floats.  save_for_backward = 1 leaves the
 * activations and edge statistics (the N rows) gcnn_backward needs in the workspace; 0 (inference) skips those stores.
 * The per-edge Dense (feature_module_final, model.py:499-500) and the upper half of output_module's first layer (model.py:505)
 * have nothing between them but the PreNorm scale (model.py:503), so the pass multiplies by their product
 * M = s2*Wf*W1a (made once per call); save_for_backward = 2 runs the two-layer form instead and also stores the tensor between
 * them (the scatter-sum output A = post_conv_module's input) -- what gcnn_prenorm_stats reads for layers 6, 8 and 10.
 * scores: [n_cuts] (model.py:300).
 * gcnn_workspace_floats returns 0 for a null dims or a negative count (every valid size is > 0); any count >= 0 is sized exactly,
 * in size_t (the calls themselves refuse more than 2^24 rows of a kind). */
size_t gcnn_workspace_floats(const gcnn_dims* dims);
int gcnn_forward(const gcnn_dims* dims, const float* params, const float* cons_feats, const float* var_feats,
                 const float* cut_feats, const gcnn_graph* cons_graph, const gcnn_graph* cut_graph,
                 float* workspace, size_t workspace_floats, float* scores, int32_t save_for_backward, void* stream);

/* ---- MSE head: MeanSquaredError on 1-D input, model_trainer.py:132,271 ----------------------------------------
 * loss_out[0] = scale * sum_k (scores_k - targets_k)^2 ; d_scores_k = 2*scale*(scores_k - targets_k).
 * scale = 1/n gives Keras' mean; data-parallel callers pass 1/global_cut_count.  loss_out / d_scores may be NULL. */
int gcnn_mse_loss(const float* scores, const float* targets, int32_t n, float scale, float* loss_out,
                  float* d_scores, void* stream);

/* ---- single-state inference: what the SCIP cut selector does per separation round, model_evaluator.py:82-111 --------
 * get_state -> ten tf.convert_to_tensor -> get_improvements(state, False).numpy() -> sorted(range(n), key=quality, reverse=True)
 * as ONE call on ONE stream: one host->device copy of the packed inputs, a three-launch graph plan specialised to a single
 * (row, col)-sorted state (utils.py:102-104), the inference forward pass, optionally the descending stable ranking of the
 * scores, one device->host copy.  Nothing is synchronised: after the call returns, wait on `stream`, then read host_out.
 *
 * host_in  (pinned): gcnn_infer_layout.in_bytes bytes; in_off[0] .. in_off[1] = a block the CALLER keeps zero (counters, flags
 *          and offset arrays of the plan ride in the upload instead of a memset), in_off[1..7] = cons_feats [C,4] f32, cons_edge_inds
 *          [2,E1] i32, cons_edge_feats [E1] f32, var_feats [V,14] f32, cut_feats [K,6] f32, cut_edge_inds [2,E2] i32,
 *          cut_edge_feats [E2] f32 (the reference's input tuple, model.py:263-275).
 * host_out (pinned): out_bytes bytes; out_off[0] scores [K] f32 (model.py:300), out_off[1] order [K] i32 (only when
 *          want_order: order[0] = index of the best cut, equal scores in index order), out_off[2] four int32 flags:
 *          [0] an edge index out of range, [1] / [2] constraint / cut edges not sorted by row, [3] a variable with more than
 *          2,048 edges.  Any flag set => the scores are NOT valid: raise on [0], otherwise use gcnn_graph_build + gcnn_forward.
 * arena    (device, 256-byte aligned, arena_bytes): inputs, plan, outputs and the forward workspace; caller-owned, reusable.
 * Returns GCNN_E_UNSUPPORTED for more than 32,768 variables (or want_order with more than 4,096 cuts), and GCNN_E_BADARG, before
 * anything is enqueued, for a state that has edges but no row or no variable they could refer to (every id of it is out of range,
 * and the plan has no row of the state's own to park such ids on). */
typedef struct gcnn_infer_layout {
    size_t in_bytes, in_off[8];
    size_t out_bytes, out_off[3];
    size_t arena_bytes, dev_off[8];   /* dev_off: internal carving of the arena behind the uploaded block */
} gcnn_infer_layout;
int gcnn_infer_layout_for(const gcnn_dims* dims, gcnn_infer_layout* layout /* host */);
int gcnn_infer(const gcnn_dims* dims, const float* params, const void* host_in, void* host_out, void* arena,
               size_t arena_bytes, int32_t want_order, void* stream);

/* Host helper of gcnn_infer (no device work): an edge list that is NOT sorted by row -- get_state emits sorted lists
 * (utils.py:102-104), other producers may not -- is brought into row order while it is packed into the staging buffer: a stable
 * counting sort (entries of a row keep their input order), O(E + n_left), a few tens of microseconds for a few 10^4 entries.
 * rows / cols / vals: the list (host); out_inds [2,E] and out_vals [E] (host, e.g. inside host_in); scratch: n_left + 1 ints (host).
 * Returns 0, or GCNN_E_BADARG when a row id lies outside [0, n_left) (nothing is written then: the device check reports it).
 * n_edges = 0 returns 0 and touches no pointer: all of them may be null then. */
int gcnn_host_sort_edges_by_row(const int32_t* rows, const int32_t* cols, const float* vals, int32_t n_edges, int32_t n_left,
                                int32_t* out_inds, float* out_vals, int32_t* scratch);
/* The packing step itself, same arguments: copies the list into the staging buffer and checks its order on the way (one pass, no
 * temporaries); a list that is not sorted by row goes through gcnn_host_sort_edges_by_row.  Returns 0 (was sorted: copied), 1
 * (sorted here), 2 (not sorted and a row id outside [0, n_left): copied as it is, the device check of gcnn_infer reports it), or
 * GCNN_E_BADARG for null pointers / negative sizes. */
int gcnn_host_pack_edges(const int32_t* rows, const int32_t* cols, const float* vals, int32_t n_edges, int32_t n_left,
                         int32_t* out_inds, float* out_vals, int32_t* scratch);

/* Keras-form Adam step (see gcnn_adam_step) to run right behind a backward pass. */
typedef struct gcnn_adam_args {
    float* params; float* m; float* v;   /* flat buffers, gcnn_param_total_floats() each; params is updated in place */
    float lr_t, beta1, beta2, eps;
} gcnn_adam_args;

/* ---- forward + loss head in one pass (the training step's forward, model_trainer.py:269-271) -------------------
 * As gcnn_forward(save_for_backward = 1); the last launch also evaluates the MSE head on its own scores,
 *   loss = loss_scale * sum_k (score_k - targets_k)^2    (loss_scale = 1/n_cuts: Keras' mean),
 * and the gradient of the readout's Dense(64->1) w.r.t. that loss, and -- the same rows, nothing in between -- the receiver-side
 * gradients of the cut rows (through the readout's hidden layer and conv v->k's update), leaving all of them in the workspace:
 * follow with gcnn_backward(d_scores = NULL, ..., loss_out), which starts at conv v->k's sender pass.  Saves the separate
 * gcnn_mse_loss launch and the first two backward launches.  (A caller that only wants loss and scores may stop here.) */
int gcnn_forward_loss(const gcnn_dims* dims, const float* params, const float* cons_feats, const float* var_feats,
                      const float* cut_feats, const gcnn_graph* cons_graph, const gcnn_graph* cut_graph,
                      float* workspace, size_t workspace_floats, float* scores, const float* targets,
                      float loss_scale, void* stream);

/* ---- backward: the vector-Jacobian product tf.GradientTape computes for GCNN.call, model_trainer.py:269-272 ----
 * d_scores: [n_cuts] gradient of the loss w.r.t. the scores; must follow gcnn_forward(save_for_backward = 1) on the same
 * workspace, inputs and parameters.  d_scores = NULL: continue from gcnn_forward_loss instead (the loss head already ran);
 * loss_out (optional) then receives that loss.  Gradients w.r.t. the 46 trainable tensors are written to `grads` (flat
 * layout; non-trainable and padding slots are left untouched -- keep them zero). */
int gcnn_backward(const gcnn_dims* dims, const float* params, const float* cons_feats, const float* var_feats,
                  const float* cut_feats, const gcnn_graph* cons_graph, const gcnn_graph* cut_graph,
                  float* workspace, size_t workspace_floats, const float* d_scores, float* grads,
                  float* cut_count_out /* optional: receives (float)n_cuts, the slot data-parallel callers all-reduce
                                          together with the gradients */,
                  float* loss_out /* optional, see above */,
                  const gcnn_adam_args* adam /* optional: apply gcnn_adam_step(params, grads, ...) right behind, fused into the
                                                last launch whenever the gradients allow it */, void* stream);

/* ---- PreNorm fitting statistics: PreNormLayer.update_params, model.py:394-423 -----------------------------------
 * For ONE batch and ONE of the 11 PreNorm layers (call order: 0 cons, 1 cons-edge, 2 var, 3 cut, 4 cut-edge, then
 * 5+2k / 6+2k = feature_module_final / post_conv_module of convolution k) writes the population mean [units] followed by
 * the mean squared deviation [units] of that layer's input to out_mean_var (device doubles; units = 4,1,14,6,1 for the
 * input layers, 1 otherwise).  Layers >= 5 read activations of a preceding gcnn_forward(save_for_backward=2) on the same
 * workspace, inputs and parameters.  The library records which form the last gcnn_forward / gcnn_forward_loss on a
 * workspace (keyed by its pointer) ran, and returns GCNN_E_BADARG instead of reading stale memory: for layers 6, 8 and 10
 * (the scatter-sum outputs A, which only save_for_backward = 2 stores) unless that forward was save_for_backward = 2, for
 * layers 5, 7 and 9 (the projections, which every form stores) unless a forward on the workspace succeeded at all.  It cannot
 * tell whether that forward had the same inputs and parameters: that stays the caller's part.
 * The streaming merge over batches (Chan et al.) is the caller's, as in the reference. */
int gcnn_prenorm_stats(const gcnn_dims* dims, const float* params, const float* cons_feats, const float* var_feats,
                       const float* cut_feats, const gcnn_graph* cons_graph, const gcnn_graph* cut_graph,
                       float* workspace, size_t workspace_floats, int32_t layer, double* out_mean_var, void* stream);

/* ---- Keras-form Adam over the flat buffer: model_trainer.py:131,273 ------------------------------------------
 * theta -= lr_t * m / (sqrt(v) + eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller (host double).
 * grad_scale (optional device scalar, may be NULL) multiplies every gradient first -- or divides it when
 * scale_is_divisor != 0 (data parallel: the all-reduced global cut count).  A divisor that is not > 0 (a global batch
 * without a single cut: model_trainer.py:271 would average over nothing) makes the call a no-op: parameters and moments
 * keep their values instead of turning into NaN. */
int gcnn_adam_step(float* params, const float* grads, float* m, float* v, int32_t n, float lr_t, float beta1,
                   float beta2, float eps, const float* grad_scale, int32_t scale_is_divisor, void* stream);

/* The same update with hyper-parameters and step counter on the device, so that a captured hipGraph of a whole training
 * step can be replayed: opt_state = {lr, beta1, beta2, eps, t, lr_t} (6 floats, device).  Each call advances t by one and
 * recomputes lr_t; the caller changes lr (the plateau schedule of model_trainer.py:177-179) by writing opt_state[0].
 * With a divisor that is not > 0 neither t nor any parameter changes (see gcnn_adam_step). */
int gcnn_adam_step_dev(float* params, const float* grads, float* m, float* v, int32_t n, float* opt_state,
                       const float* grad_scale, int32_t scale_is_divisor, void* stream);

/* ---- ranking-prefix accuracy on the device: model_trainer.py:280-302 / model_tester.py:205-224 ----------------------
 * Per sample s (cuts offsets[s] .. offsets[s+1]-1 of the stacked vectors): rank by pred and by truth, descending, ties in
 * index order (Python's stable sorted(reverse=True)); frac = first differing position / #cuts (1 if none).
 * acc[f] += [frac >= fractions[f]] (accumulates across calls); frac_out[s] = frac (optional).  max_cuts = largest sample
 * (host value, <= 4096, else GCNN_E_WORKSPACE).  Optionally also accumulates the cut-weighted loss of
 * model_trainer.py:304: loss_acc[0] += loss_in[0] * loss_weight. */
int gcnn_ranking_metric(const float* pred, const float* truth, const int32_t* offsets, int32_t n_samples,
                        int32_t max_cuts, const float* fractions, int32_t n_fractions, float* acc, float* frac_out,
                        const float* loss_in, float loss_weight, float* loss_acc, void* stream);

/* ---- cut selection: the parallelism filter of the SCIP plugin's cutselselect, model_evaluator.py:109-154 ----------------
 * (the same loop: model_benchmarker.py:112-157, data_collector.py:150-195).  Per sample s (cuts cut_offsets[s] .. [s+1]-1 of the
 * stacked vectors, forced rows forced_offsets[s] .. [s+1]-1), all in STATE order (cut k = row k of cut_feats / cut_edge_inds):
 *   order   = the descending stable ranking of quality (NaN as -inf): what gcnn_infer's order holds;
 *   low[p]  = quality[order[p]] < t in fp32, t = (float)(0.9 * (double)quality[order[0]]) -- fixed by POSITION p;
 *   P(x,y)  = |sum_v x_v y_v| over the rows as dense vectors (duplicate entries add), accumulated in fp64; 0 for an empty row
 *             (get_state stores each cut row divided by its norm, utils.py:214-236, so this is SCIP's row parallelism);
 *   a cut at position p is removed by pivot row r when P > p_max and (low[p] or P > p_max_ub);
 *   forced phase: for each forced row in order, the removed positions among [0, n) move behind all others (position order kept
 *   on both sides) and n shrinks; main phase: for i = 0, 1, ... while i < n - 1, the same with pivot order[i] and the positions
 *   (i, n).  Output: order[] (sample-local cut indices, at the sample's cut offset) and n_kept[s] = n (-1 when the sample has
 *   more than max_cuts cuts).
 * quality: [total_cuts] any score vector (device).  cut_ptr / cut_col / cut_val: the cut rows as by-left CSR (a gcnn_graph's
 * l_ptr / l_oth / l_coef); forced_ptr / forced_col / forced_val: the forced rows in the same form and column space (row offsets
 * over the stacked forced rows; NULL when total_forced = 0).  Entries whose column lies outside [0, n_vars) take no part.
 * cut_offsets / forced_offsets: [n_samples+1] device int32, or NULL for n_samples = 1.  max_cuts: the largest sample (host value,
 * <= 4096, else GCNN_E_UNSUPPORTED).  p_max, p_max_ub: finite, else GCNN_E_BADARG.  workspace: gcnn_select_workspace_bytes
 * (the two parallelism bits of every pair the filter can consult).  Two launches; nothing is synchronised. */
size_t gcnn_select_workspace_bytes(int32_t total_cuts, int32_t total_forced, int32_t max_cuts);
int gcnn_select_cuts(const float* quality, const int32_t* cut_ptr, const int32_t* cut_col, const float* cut_val,
                     const int32_t* cut_offsets, int32_t n_samples, int32_t total_cuts, int32_t max_cuts, int32_t n_vars,
                     const int32_t* forced_ptr, const int32_t* forced_col, const float* forced_val,
                     const int32_t* forced_offsets, int32_t total_forced, double p_max, double p_max_ub, int32_t* order,
                     int32_t* n_kept /* [n_samples] */, void* workspace, size_t workspace_bytes, void* stream);

/* Single call: gcnn_infer (want_order) followed by gcnn_select_cuts on its scores and on the cut rows already in the arena, with
 * ONE upload (the packed state of gcnn_infer, then the forced rows) and ONE download (scores | order | flags | n_kept).
 * layout.infer: as gcnn_infer_layout_for, except that in_bytes / out_bytes / arena_bytes cover this call.  host_in additionally
 * holds forced_off[0]: forced_ptr [n_forced+1] int32 (offsets from 0), forced_off[1]: forced_col [n_forced_entries] int32,
 * forced_off[2]: forced_val [n_forced_entries] f32.  host_out additionally holds n_kept (int32) at n_kept_off.  The flags are those
 * of gcnn_infer: any set => scores and selection are NOT valid; the caller takes the general path (gcnn_graph_build +
 * gcnn_forward + gcnn_select_cuts).  Returns GCNN_E_UNSUPPORTED for more than 32,768 variables or 4,096 cuts. */
typedef struct gcnn_select_layout {
    gcnn_infer_layout infer;
    size_t forced_off[3];
    size_t n_kept_off;
    size_t ws_off;            /* internal: the selection workspace inside the arena */
} gcnn_select_layout;
int gcnn_infer_select_layout_for(const gcnn_dims* dims, int32_t n_forced, int32_t n_forced_entries,
                                 gcnn_select_layout* layout /* host */);
int gcnn_infer_select(const gcnn_dims* dims, int32_t n_forced, int32_t n_forced_entries, const float* params,
                      const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max, double p_max_ub,
                      void* stream);

/* ---- groups: several independent models stepped in one set of launches ---------------------------------------------------
 * A group is 1..GCNN_GROUP_MAX models (e.g. the seeds of model_trainer.py:38-49), each with its own parameters, batch,
 * workspace, gradients and Adam state.  gcnn_group_train_step runs, for every member, exactly what gcnn_forward_loss followed
 * by gcnn_backward(d_scores = NULL, cut_count_out = NULL, loss_out, adam) runs -- with the same bits -- but stage by stage for
 * all members in one launch per distinct kernel (same-shaped members: the launch count of one solo step).  gcnn_group_forward
 * does the same for gcnn_forward(save_for_backward = 0): scores only.  A member with no constraint, variable or cut takes the
 * solo entry points inside the call.
 * host_staging (host, pinned, 16-B aligned) and device_table (64-B aligned): gcnn_group_table_bytes(n) bytes each.  The call
 * builds every launch table of the step in host_staging and uploads them with ONE hipMemcpyAsync on `stream`: host_staging must
 * not be rewritten (by another group call) before that copy has run -- give back-to-back calls different staging buffers, or
 * wait for an event recorded behind the call.  device_table may be reused by the next call on the same stream.
 * Checked before anything is enqueued: n out of 1..GCNN_GROUP_MAX or buffers missing -> GCNN_E_BADARG; a workspace or the table
 * too small -> GCNN_E_WORKSPACE; two members whose writable buffers (workspace, scores; training: grads, loss_out and the
 * Adam params, m, v) overlap -> GCNN_E_BADARG.  Read-only inputs (parameters without an update, features, graphs, targets)
 * may be shared. */
#define GCNN_GROUP_MAX 8
typedef struct gcnn_group_member {
    gcnn_dims dims;
    const float* params;
    const float *cons_feats, *var_feats, *cut_feats;
    gcnn_graph cons_graph, cut_graph;
    float* workspace; size_t workspace_floats;
    float* scores;                 /* [n_cuts] */
    const float* targets;          /* training: [n_cuts] */
    float loss_scale;              /* training: as gcnn_forward_loss */
    float* grads;                  /* training: flat gradient buffer */
    float* loss_out;               /* training, optional: [1] */
    const gcnn_adam_args* adam;    /* training, optional (host struct): NULL = no update */
} gcnn_group_member;
int gcnn_group_table_bytes(int32_t n_members, size_t* bytes /* host */);
int gcnn_group_train_step(int32_t n_members, const gcnn_group_member* members /* host */, void* host_staging, void* device_table,
                          size_t table_bytes, void* stream);
int gcnn_group_forward(int32_t n_members, const gcnn_group_member* members /* host */, void* host_staging, void* device_table,
                       size_t table_bytes, void* stream);

/* ---- PreNorm fitting with the streaming merge on the device: GCNN.pretrain without a host read per batch --------------------
 * gcnn_prenorm_merge: for ONE batch and ONE PreNorm layer (numbered as in gcnn_prenorm_stats), everything GCNN.pretrain does with
 * the batch -- for layers >= 5 the gcnn_forward(save_for_backward = 2) it reads (its scores land in the workspace), then
 * gcnn_prenorm_stats' two statistics passes (the same grids, so the same fp64 sums), then the streaming merge (Chan et al.,
 * model.py:415-423) of the batch's mean and variance into `state`, in fp32 and rounded as NumPy rounds it: bit for bit the
 * host merge of GCNN.pretrain.  `state`: GCNN_PRENORM_STATE_BYTES of device memory, 8-B aligned, zeroed before the first batch
 * of a layer and read after the last: the fp32 count at byte 0, mean [units] at GCNN_PRENORM_STATE_MEAN and var [units] at
 * GCNN_PRENORM_STATE_VAR (the rest is scratch).  A batch with nothing to absorb (the layer's input is empty: known from the
 * dims, so the caller may skip the call) enqueues nothing and leaves the state as it was.  Arguments are checked as
 * gcnn_prenorm_stats checks them.
 * gcnn_group_prenorm_merge: the same for up to GCNN_GROUP_MAX models in one set of launches, member i on layers[i] (host) into
 * states[i] (host array of device pointers), recorded and launched as gcnn_group_forward is (the members' scores, targets,
 * grads, loss_out and adam are not used).  Every state gets the bits gcnn_prenorm_merge gives it.  Staging, table and checks
 * as gcnn_group_forward, and also GCNN_E_BADARG (nothing enqueued) for a layer outside 0..10, a missing or misaligned state, or
 * a state that overlaps any buffer of another member. */
#define GCNN_PRENORM_STATE_BYTES 272
#define GCNN_PRENORM_STATE_MEAN 16
#define GCNN_PRENORM_STATE_VAR 80
int gcnn_prenorm_merge(const gcnn_dims* dims, const float* params, const float* cons_feats, const float* var_feats,
                       const float* cut_feats, const gcnn_graph* cons_graph, const gcnn_graph* cut_graph,
                       float* workspace, size_t workspace_floats, int32_t layer, void* state, void* stream);
int gcnn_group_prenorm_merge(int32_t n_members, const gcnn_group_member* members /* host */, const int32_t* layers /* host */,
                             void* const* states /* host */, void* host_staging, void* device_table, size_t table_bytes,
                             void* stream);

/* ---- test stage: rankings of many candidates against one truth (model_tester.py:113-153, 205-224) --------------------------
 * For every sample s (cuts offsets[s] .. offsets[s+1]-1; K_total = offsets[n_samples] is the row stride of scores and perms), the
 * first position at which a candidate ranking deviates from the truth ranking.  Rankings are stable descending orders (Python's
 * sorted(..., reverse=True): ties in index order), NaN ranked as -inf.  Output rows of deviations [rows][n_samples], int32:
 *   0 .. n_scores-1       scores [n_scores][K_total] fp32 against truth32 [K_total] fp32
 *   n_scores              hybrid [K_total] fp64, when not NULL, against truth64 [K_total] fp64
 *   then n_perms rows     perms [n_perms][K_total] int32 (perm[r] = the sample-local cut at rank r) against truth64
 * Each value: the first deviating position; the number of cuts when the rankings agree; 0 for a sample without cuts; -1 for a
 * sample with more than 4,096 cuts (restate it on the host).  fp64 keys are compared in fp64.  All pointers are device memory.
 * One launch.  GCNN_E_BADARG (nothing enqueued) for n_samples < 1, n_scores or n_perms outside 0..GCNN_GROUP_MAX, no candidate
 * at all, or a missing pointer: offsets, deviations; truth32 and scores when n_scores > 0; perms when n_perms > 0; truth64 when
 * hybrid or perms are given. */
int gcnn_rank_deviations(const int32_t* offsets, int32_t n_samples, const float* truth32, const double* truth64,
                         const float* scores, int32_t n_scores, const double* hybrid, const int32_t* perms, int32_t n_perms,
                         int32_t* deviations, void* stream);

/* ---- many host states in one call: the evaluators' task farms (model_evaluator.py:157-241) behind one GPU process ---------------
 * gcnn_infer's contract -- ONE host->device copy of a packed pinned buffer, ONE device->host copy, nothing synchronised, nothing
 * allocated -- for 1..GCNN_IBATCH_MAX states at once, scored as their disjoint union (utils.py:389-426) in ONE forward pass.
 * Every state comes with STATE-LOCAL indices; the device shifts them.  dims[s]: the sizes of state s; n_forced[s] /
 * n_forced_entries[s]: its forced rows (may be NULL = none; only GCNN_IBATCH_SELECT reads forced rows).
 *
 * host_in (pinned), with O = in_off and c/v/k/e1/e2/f/fe_off[s] = the exclusive prefix sums of the states' sizes:
 *   O[0]  the table: GCNN_IBATCH_TABLE_COLS columns of GCNN_IBATCH_TABLE_STRIDE int32 -- c_off, v_off, k_off, e1_off, e2_off,
 *         f_off, fe_off, entries 0..n_states (the last = the total); gcnn_infer_batch_fill_table writes it
 *   O[1]  a block the CALLER keeps zero up to O[2] (per-state flags and the by-left offsets of both edge sets)
 *   O[2]  cons_feats [C,4]: state s at row c_off[s]            O[5]  var_feats [V,14]     O[6]  cut_feats [K,6]
 *   O[3]  constraint edges: state s's own [2,E1_s] int32 block at int32 position 2*e1_off[s] (what gcnn_host_pack_edges writes)
 *   O[4]  cons_edge_feats [E1]: state s at e1_off[s]           O[7], O[8]  the cut edges in the same two forms
 *   O[9]  forced_ptr [F+1] int32: offsets over the STACKED forced entries (state s's own offsets + fe_off[s])
 *   O[10] forced_col [FE] int32, state-local column ids        O[11] forced_val [FE] f32
 * host_out (pinned): out_off[0] scores [K] (state s at k_off[s]), out_off[1] order [K] int32 (state-local cut indices at k_off[s];
 *   RANK: the descending stable ranking, NaN as -inf; SELECT: as gcnn_select_cuts), out_off[2] n_kept [n_states] int32 (SELECT
 *   only; -1 for a state with more than 4,096 cuts), out_off[3] flags [n_states][4] int32 with the meaning of gcnn_infer's flags
 *   ([3] stays 0: the by-variable order is a stable radix sort of the union's list and knows no degree limit).
 * A state with a flag set has no valid scores, order or n_kept; neither has, in RANK / SELECT, the order of a state with more than
 * 4,096 cuts.  Such a state does not change any other state's results: its bad ids are replaced inside its own index ranges and a
 * disjoint union shares no node between states.  The caller re-runs it alone (gcnn_infer, or gcnn_graph_build + gcnn_forward).
 * Returned before anything is enqueued: GCNN_E_BADARG for n_states outside 1..GCNN_IBATCH_MAX, a negative size, an unknown mode or
 * a threshold that is not finite; GCNN_E_UNSUPPORTED for a union of more than 2^24 rows of one kind or 2^30 edges of one set, and
 * for a state that has edges but no row or no variable they could refer to (every id of it would be out of range). */
#define GCNN_IBATCH_MAX 64
#define GCNN_IBATCH_TABLE_COLS 7
#define GCNN_IBATCH_TABLE_STRIDE 72
#define GCNN_IBATCH_SCORES 0
#define GCNN_IBATCH_RANK 1
#define GCNN_IBATCH_SELECT 2
typedef struct gcnn_ibatch_layout {
    gcnn_dims total;                       /* the union's sizes */
    int32_t n_forced, n_forced_entries;    /* totals */
    int32_t max_cuts;                      /* the largest state that takes part in RANK / SELECT (<= 4,096) */
    int32_t n_states;
    size_t in_bytes, in_off[12];
    size_t out_bytes, out_off[4];
    size_t arena_bytes, dev_off[16];       /* dev_off: internal carving of the arena behind the uploaded block */
} gcnn_ibatch_layout;
int gcnn_infer_batch_layout_for(int32_t n_states, const gcnn_dims* dims /* host [n_states] */, const int32_t* n_forced,
                                const int32_t* n_forced_entries, int32_t mode, gcnn_ibatch_layout* layout /* host */);
/* table: host_in + in_off[0] (host).  No device work. */
int gcnn_infer_batch_fill_table(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced,
                                const int32_t* n_forced_entries, int32_t* table /* host */);
int gcnn_infer_batch(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                     int32_t mode, const float* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes,
                     double p_max, double p_max_ub, void* stream);

/* ---- the state from a raw LP snapshot: the arithmetic of get_state (utils.py:35-238) on the device ---------------------------------
 * get_state walks solver objects AND turns what it finds into the model's inputs.  Only the walk is solver-bound; these entry
 * points do the rest.  The caller hands over the LP as the solver holds it -- float64 values, int32 indices, int8 codes --
 *   rows  (R):  CSR row_ptr [R+1], row_col [nnz] (LP column positions), row_val [nnz]; row_lhs, row_rhs, row_dual [R];
 *               row_basis [R]: 0 lower, 1 basic, 2 upper, 3 zero
 *   cols  (V):  col_type [V]: 0 binary, 1 integer, 2 implicit integer, 3 continuous; col_obj, col_lb, col_ub [V]; col_basis [V];
 *               col_lp, col_redcost [V]; with an incumbent also col_primal and col_primal_avg [V]
 *   cuts  (K):  CSR cut_ptr [K+1], cut_col, cut_val; cut_lhs, cut_rhs [K]
 * packed into ONE buffer at gcnn_lp_layout.snap_off, in the order of GCNN_LP_* below; snap_off[GCNN_LP_HEADER] is a reserved 16-byte block
 * (not read).  The snapshot is read only: violations are noted in the scratch, so one device snapshot may serve several calls.
 * Contract: within a row or cut the columns are strictly increasing (scipy's sum_duplicates(), utils.py:102,226),
 * every cut has an entry, constants are already moved into lhs / rhs.  "finite" below means not |x| >= infinity.
 * The device writes the reference's input tuple (model.py:263-275), in get_state's layout and order:
 *   constraints: every row with a finite lhs, in LP order, negated: [-lhs/norm, basis == lower, -cosine, -dual], then every row with a
 *     finite rhs: [rhs/norm, basis == upper, cosine, dual]; norm = sqrt(sum a^2) (0 -> 1), cosine = a.obj/(norm*obj_norm), dual =
 *     row_dual/(norm*obj_norm).  C = #lhs + #rhs (equality and ranged rows appear twice); edges -a/norm | a/norm, (row, col)-sorted.
 *   variables:   one-hot type, obj/obj_norm, has_lb, has_ub, basis == lower, basis == upper, 0.5 - |x - floor(x) - 0.5| (0 when
 *     continuous), redcost/obj_norm, lp, primal, primal_avg (zeros without an incumbent)            (utils.py:118-159)
 *   cuts:        activity = a.col_lp; a cut takes its lhs side iff lhs is finite and lhs - activity > activity - rhs; lhs-side cuts
 *     first, then rhs-side cuts, each group in input order (utils.py:180-185): [-lhs/norm | rhs/norm, nnz/n_model_vars,
 *     #non-continuous columns/nnz, efficacy, cutoff, parallelism]; edges as for rows.  With feasibility = min(rhs - activity,
 *     activity - lhs): efficacy = -feasibility/norm; cutoff = 0 without an incumbent, else with d = a.(col_primal - col_lp) /
 *     |col_primal - col_lp| (0 when that norm is 0), |d| <= sum_epsilon replaced by copysign(sum_epsilon, d): min(-feasibility/|d|,
 *     infinity); parallelism = |a.col_obj|/(|a|*|col_obj|), 0 when the product is 0.  (This project's reading of SCIP's
 *     getCutEfficacy, getCutLPSolCutoffDistance and getRowObjParallelism at default settings: DESIGN.md section 7.)
 *   cut_index [K] int32: state position -> input cut.
 * Sums, divisions and square roots are fp64, each output is rounded to fp32 once; no float atomics: the same bits from run to run.
 * n_state_rows (C) and n_state_edges (E1) are the caller's: count the rows with a finite lhs / rhs and their entries (O(R)); the
 * device recomputes both and reports a difference.  flags [4] int32 (device): [0] a column outside [0, n_cols), [1] columns of a row
 * or cut not strictly increasing, [2] offsets not monotone inside [0, nnz], [3] C or E1 differ from the device's count.  Any flag
 * set => the state is NOT valid.  Whatever the snapshot holds, no kernel reads or writes outside the arrays as sized by the dims. */
typedef struct gcnn_lp_dims {
    int32_t n_rows, n_cols, n_cuts, row_nnz, cut_nnz;
    int32_t has_incumbent;
    int32_t n_model_vars;                  /* getNVars() of utils.py:188; >= 1 */
    int32_t n_state_rows, n_state_edges;   /* C, E1 */
    int32_t reserved;
    double infinity, sum_epsilon;          /* SCIP defaults: 1e20, 1e-6 */
    double obj_norm;                       /* > 0: the objective's norm, a value <= 0 already replaced by 1 (utils.py:50-51) */
} gcnn_lp_dims;
#define GCNN_LP_ARRAYS 22
enum { GCNN_LP_HEADER = 0, GCNN_LP_ROW_PTR, GCNN_LP_ROW_COL, GCNN_LP_ROW_VAL, GCNN_LP_ROW_LHS, GCNN_LP_ROW_RHS, GCNN_LP_ROW_DUAL,
       GCNN_LP_ROW_BASIS, GCNN_LP_COL_TYPE, GCNN_LP_COL_OBJ, GCNN_LP_COL_LB, GCNN_LP_COL_UB, GCNN_LP_COL_BASIS, GCNN_LP_COL_LP,
       GCNN_LP_COL_REDCOST, GCNN_LP_COL_PRIMAL, GCNN_LP_COL_PRIMAL_AVG, GCNN_LP_CUT_PTR, GCNN_LP_CUT_COL, GCNN_LP_CUT_VAL,
       GCNN_LP_CUT_LHS, GCNN_LP_CUT_RHS };
/* gcnn_lp_layout_for fills snap_* and scratch_bytes for every valid dims (what gcnn_lp_state needs), and the single call's part
 * when the sizes are inside gcnn_infer's limits (call_supported = 1).  n_forced < 0: the layout of gcnn_lp_infer; >= 0: that of
 * gcnn_lp_infer_select with so many forced rows / entries. */
typedef struct gcnn_lp_layout {
    size_t snap_bytes, snap_off[GCNN_LP_ARRAYS];
    size_t scratch_bytes;
    int32_t call_supported, reserved;
    size_t in_bytes, forced_off[3];        /* host_in: the packed snapshot, then forced_ptr | forced_col | forced_val as in gcnn_infer_select */
    size_t out_bytes, out_off[6];          /* host_out: scores [K] f32 | order [K] i32 | gcnn_infer's 4 flags | n_kept | the 4 LP flags | cut_index [K] */
    size_t arena_bytes, ws_off, lp_off, scratch_off;   /* internal carving of the arena */
    gcnn_infer_layout state;               /* internal: where the state, the plan and the forward workspace live in the arena */
} gcnn_lp_layout;
int gcnn_lp_layout_for(const gcnn_lp_dims* dims, int32_t n_forced, int32_t n_forced_entries, gcnn_lp_layout* layout /* host */);
/* snapshot (device, 16-byte aligned, packed at snap_off) -> the seven arrays and cut_index in device memory (cons_feats 16-byte
 * aligned), on `stream`; two launches, nothing synchronised.  scratch: scratch_bytes of device memory, 16-byte aligned. */
int gcnn_lp_state(const gcnn_lp_dims* dims, const void* snapshot, void* scratch, size_t scratch_bytes, float* cons_feats,
                  int32_t* cons_edge_inds /* [2,E1] */, float* cons_edge_feats, float* var_feats, float* cut_feats,
                  int32_t* cut_edge_inds /* [2,E2] */, float* cut_edge_feats, int32_t* cut_index, int32_t* flags /* [4] */,
                  void* stream);
/* gcnn_infer / gcnn_infer_select on a snapshot: ONE upload of host_in (pinned, in_bytes), the two state-building launches write the
 * seven arrays where gcnn_infer's upload would have put them, then the same plan, forward pass and ranking / selection, ONE
 * download of host_out (pinned, out_bytes).  Scores and order are in STATE order: map them through cut_index.  Any of the eight
 * flags set => nothing else in host_out is valid (an LP flag, or gcnn_infer's [0]: bad input; gcnn_infer's [1..3]: build the state
 * with gcnn_lp_state and take gcnn_graph_build + gcnn_forward).  GCNN_E_UNSUPPORTED where gcnn_infer / gcnn_infer_select return it. */
int gcnn_lp_infer(const gcnn_lp_dims* dims, const float* params, const void* host_in, void* host_out, void* arena,
                  size_t arena_bytes, int32_t want_order, void* stream);
int gcnn_lp_infer_select(const gcnn_lp_dims* dims, int32_t n_forced, int32_t n_forced_entries, const float* params,
                         const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max, double p_max_ub,
                         void* stream);

/* ---- many LP snapshots in one call: gcnn_infer_batch in front of which the device builds every state ------------------------------
 * What a scoring server does with the LP snapshots that queued up (model_evaluator.py:157-241: one selector call per worker and
 * separation round): 1..GCNN_IBATCH_MAX snapshots in ONE host->device copy, two launches that run gcnn_lp_state's arithmetic for all
 * of them and leave state s exactly where gcnn_infer_batch's upload would have put it (features at the union's rows, each edge list as
 * the state's own [2,E_s] block with state-local ids), then gcnn_infer_batch's index pass, by-variable sort, ONE forward pass and
 * ranking / selection unchanged, ONE device->host copy.  Nothing is synchronised, nothing allocated.  Every state has the bits
 * gcnn_lp_state gives it alone.  There is no variable limit (gcnn_lp_infer's 32,768 is the single-state plan's).
 * dims[s]: snapshot s as gcnn_lp_state takes it; n_forced[s] / n_forced_entries[s] and mode as in gcnn_infer_batch.
 *
 * host_in (pinned, in_bytes): [0, table_bytes) the tables -- gcnn_lp_batch_fill_table writes them: the union's table of
 *   gcnn_infer_batch, then one descriptor per snapshot (sizes, scalars, where its arrays, scratch and outputs lie in the arena as
 *   byte positions from the arena's start, its first block in either launch); snapshot s packed as gcnn_lp_layout_for(dims[s]) says, its
 *   array i at snap_base[s] + snap_off[i]; forced_off[0..2]: forced_ptr | forced_col | forced_val as gcnn_infer_batch's O[9..11].
 * host_out (pinned, out_bytes): out_off[0..3] as gcnn_infer_batch's (scores, order, n_kept, flags [n][4]); out_off[4] the LP flags
 *   [n][4] of gcnn_lp_state; out_off[5] cut_index [K] int32, state s at k_off[s], state-local.  Scores and order are in STATE order.
 * A snapshot with an LP flag set has no valid results and changes no other snapshot's: it leaves parts of its own state unwritten,
 * and whatever ids lie there are confined to its own ranges (gcnn_infer_batch).  Otherwise the four batch flags decide as there.
 * state: the union's layout for the built states' sizes: in_off[1] the zero block (cleared by the first launch) and in_off[2..8] the
 *   seven arrays, inside the arena; nothing of it is uploaded.
 * Returned before anything is enqueued: what gcnn_infer_batch returns for the built states' sizes (n outside 1..GCNN_IBATCH_MAX, a
 * union past 2^24 rows or 2^30 edges, edges with nothing to point at, thresholds, buffers), and GCNN_E_BADARG for a gcnn_lp_dims
 * gcnn_lp_layout_for refuses. */
typedef struct gcnn_lp_batch_layout {
    gcnn_ibatch_layout state;
    int32_t n_snapshots, reserved;
    size_t table_bytes;
    size_t in_bytes, snap_base[GCNN_IBATCH_MAX], forced_off[3];
    size_t out_bytes, out_off[6];
    size_t arena_bytes, up_off, out_dev_off, scratch_off, scratch_base[GCNN_IBATCH_MAX];   /* internal carving of the arena */
} gcnn_lp_batch_layout;
int gcnn_lp_batch_layout_for(int32_t n, const gcnn_lp_dims* dims /* host [n] */, const int32_t* n_forced,
                             const int32_t* n_forced_entries, int32_t mode, gcnn_lp_batch_layout* layout /* host */);
/* table: host_in (host), table_bytes bytes.  No device work. */
int gcnn_lp_batch_fill_table(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                             int32_t mode, void* table /* host */);
int gcnn_lp_batch(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int32_t mode,
                  const float* params, const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max,
                  double p_max_ub, void* stream);

/* ---- hybrid cut selection from cut rows: SCIP's hybrid quality and the parallelism filter, no LP rows, no model -----------------
 * The `function=None` arm of the reference's selector (model_evaluator.py:104-154), the baseline arm of model_benchmarker.py and
 * every non-expert round of data_collector.py:145-195, for 1..GCNN_IBATCH_MAX snapshots in ONE host->device copy, at most four
 * launches whatever n is, ONE device->host copy.  Nothing is synchronised, nothing allocated.
 * Input per snapshot (the gcnn_lp_state contract for these fields): the cuts as CSR over LP column positions (cut_ptr, cut_col,
 * cut_val, cut_lhs, cut_rhs; columns strictly increasing within a cut, every cut has an entry, constants already in lhs / rhs), the
 * columns' col_type, col_obj, col_lp, and `infinity`.
 * Per cut, in fp64: sum a^2, act = a.lp, a.obj and nint (columns of type != 3) exactly as gcnn_lp_state adds them (16 lanes a cut),
 * |obj| exactly as it adds it (256-column chunks, the chunk sums strided over 256 threads, a block tree); then
 *   efficacy    = -min(rhs - act, act - lhs) / norm,  norm = sqrt(sum a^2), or 1 when that is 0
 *   int_support = nint / nnz
 *   parallelism = 0 when sqrt(sum a^2) * |obj| = 0, else |a.obj| / (sqrt(sum a^2) * |obj|)
 * -- the doubles gcnn_lp_state rounds into cut_feats[:, 3], [:, 2] and [:, 5] -- and
 *   quality     = (efficacy + (0.1 * nint) / nnz) + 0.1 * parallelism
 * with every operation rounded on its own in this association (Python's evaluation of the reference's line; no fused multiply-add).
 * The rows of the filter are cut_val / norm rounded to fp32, in INPUT cut order with their columns as given: get_state's stored
 * rows up to a sign that |a.b| removes.  The selection is gcnn_select_cuts' with a float64 key: order = the descending stable
 * ranking of quality (NaN as -inf, ties in input order), low[p] = quality[order[p]] < 0.9 * quality[order[0]] compared in fp64 (no
 * fp32 rounding of the threshold: the plugin's quality array is float64 here), forced phase and main phase as there.  All outputs
 * are in input cut order.
 * mode: GCNN_HYBRID_QUALITY (quality and features; two launches), GCNN_HYBRID_RANK (also order = the ranking, n_kept = n_cuts;
 * three), GCNN_HYBRID_SELECT (the selection; four).  Forced rows (GCNN_HYBRID_SELECT only; n_forced may be NULL = none) as
 * gcnn_infer_batch takes them.
 *
 * host_in (pinned, in_bytes): [0, table_bytes) the table, written by gcnn_hybrid_fill_table; array i of snapshot s at
 *   snap_off[s][i] in the order GCNN_HYBRID_CUT_PTR .. GCNN_HYBRID_COL_LP (int32, int32, f64, f64, f64, int8, f64, f64);
 *   forced_off[0..2]: forced_ptr [F+1] int32 (offsets over the stacked entries of all snapshots) | forced_col | forced_val f32.
 * host_out (pinned, out_bytes): out_off[0] quality f64 [total_cuts] | out_off[1] features f64 [total_cuts][3] (efficacy,
 *   int_support, parallelism) | out_off[2] order int32 [total_cuts], snapshot-local | out_off[3] n_kept int32 [n] | out_off[4] flags
 *   int32 [n][4]: words 0-2 as gcnn_lp_state's (a column out of range, columns not strictly increasing, offsets not monotone), word 3
 *   is 0.  Snapshot s starts at cut c_off[s] = n_cuts[0] + .. + n_cuts[s-1].  A flagged snapshot has no valid results and changes
 *   no other snapshot's bits.
 * Returned before anything is enqueued: GCNN_E_BADARG for n outside 1..GCNN_IBATCH_MAX, a negative size, an infinity that is not
 * positive, an unknown mode, forced entries without a row, a missing buffer, an arena shorter than arena_bytes or not 256-byte
 * aligned, or (GCNN_HYBRID_SELECT) a threshold that is not finite; GCNN_E_UNSUPPORTED for a snapshot of more than 4,096 cuts when
 * an order is wanted, or a union of more than 2^30 cuts or entries. */
#define GCNN_HYBRID_ARRAYS 8
#define GCNN_HYBRID_CUT_PTR 0
#define GCNN_HYBRID_CUT_COL 1
#define GCNN_HYBRID_CUT_VAL 2
#define GCNN_HYBRID_CUT_LHS 3
#define GCNN_HYBRID_CUT_RHS 4
#define GCNN_HYBRID_COL_TYPE 5
#define GCNN_HYBRID_COL_OBJ 6
#define GCNN_HYBRID_COL_LP 7
#define GCNN_HYBRID_QUALITY 0
#define GCNN_HYBRID_RANK 1
#define GCNN_HYBRID_SELECT 2
typedef struct gcnn_hybrid_dims {
    int32_t n_cols, n_cuts, cut_nnz, reserved;
    double infinity;
} gcnn_hybrid_dims;
typedef struct gcnn_hybrid_layout {
    int32_t n_snapshots, total_cuts, total_nnz, max_cuts, max_cols, n_forced, n_forced_entries, reserved;
    size_t table_bytes, in_bytes, snap_off[GCNN_IBATCH_MAX][GCNN_HYBRID_ARRAYS], forced_off[3];
    size_t out_bytes, out_off[5];
    size_t arena_bytes, out_dev_off, rows_off[3], ws_off, scratch_off, scratch_base[GCNN_IBATCH_MAX];   /* internal carving of the arena (the upload lies at 0) */
} gcnn_hybrid_layout;
int gcnn_hybrid_layout_for(int32_t n, const gcnn_hybrid_dims* dims /* host [n] */, const int32_t* n_forced,
                           const int32_t* n_forced_entries, int32_t mode, gcnn_hybrid_layout* layout /* host */);
/* table: host_in (host), table_bytes bytes.  No device work. */
int gcnn_hybrid_fill_table(int32_t n, const gcnn_hybrid_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                           int32_t mode, void* table /* host */);
int gcnn_hybrid_select(int32_t n, const gcnn_hybrid_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                       int32_t mode, const void* host_in, void* host_out, void* arena, size_t arena_bytes, double p_max,
                       double p_max_ub, void* stream);

/* ---- the data collector's expert round: the sample's state and the selection over the caller's quality, in one call ---------------
 * data_collector.SamplingAgent.cutselselect (data_collector.py:86-195) in a round that queries the expert: SCIP's dives give a
 * float64 quality per cut (data_collector.py:104-131); the plugin then needs get_state(model, cuts) for the sample
 * (data_collector.py:135-136) and its ranking and parallelism filter over that quality (data_collector.py:150-195).  gcnn_lp_collect
 * replaces both: ONE host->device copy, at most six launches, ONE device->host copy; nothing is synchronised, nothing allocated.
 *   the state      gcnn_lp_state's two launches write the seven arrays, cut_index and the four LP flags into the download block;
 *   the rows       gcnn_hybrid_select's two row-building launches, on a one-entry table whose eight array positions point into
 *                  the uploaded LP snapshot (cut_ptr, cut_col, cut_val, cut_lhs, cut_rhs, col_type, col_obj, col_lp; `infinity`
 *                  from dims): cut_val / norm in fp32, INPUT cut order -- and with them the hybrid quality and features of
 *                  gcnn_hybrid_select, the plugin's fallback ranking (data_collector.py:145-148), for free;
 *   the selection  gcnn_select_cuts' pair launch on those rows and the forced rows, then gcnn_hybrid_select's fp64 filter with the
 *                  UPLOADED quality as its key: order = sorted(range(K), key=lambda x: quality[x], reverse=True) over INPUT cut
 *                  indices (ties in input order), low[p] = quality[order[p]] < 0.9 * quality[order[0]] in fp64, forced phase,
 *                  main phase.  order and n_kept are in input cut indices; the state is in get_state's order (lhs-side cuts
 *                  first), so the sample's labels are quality[cut_index[p]] for state position p.
 * quality must be finite (the reference records a sample only when every dive solved: the caller checks; NaN ranks as -inf here).
 * n_forced >= 0 (0: none), forced rows as gcnn_infer_select takes them.
 * host_in (pinned, 16-byte aligned, in_bytes; WRITTEN: the call puts its table at table_off before the copy): the LP snapshot packed
 *   at snap_off as gcnn_lp_layout_for says | quality_off: quality [K] f64 | forced_off[0..2]: forced_ptr | forced_col | forced_val |
 *   table_off.  in_bytes = gcnn_lp_layout_for(dims, n_forced, n_forced_entries).in_bytes + 8 * K rounded up to 16 + table_bytes.
 * host_out (pinned, out_bytes), at out_off[GCNN_LP_COLLECT_*]: cons_feats [C,4] | cons_edge_inds [2,E1] | cons_edge_feats [E1] |
 *   var_feats [V,14] | cut_feats [K,6] | cut_edge_inds [2,E2] | cut_edge_feats [E2] | cut_index [K] int32 | LP flags [4] |
 *   hybrid quality [K] f64 | features [K][3] f64 | order [K] int32 | n_kept int32 | hybrid flags [4] (words 0-2 as the LP flags').
 *   Any flag set => nothing else is valid.
 * entry_snap: the eight positions the table's entry holds, = snap_off of the corresponding LP arrays (the upload lies at the arena's
 *   start).  The scratch of both families is carved out of the arena, so GCNN_E_WORKSPACE does not arise.
 * Returned before anything is enqueued: GCNN_E_BADARG for dims gcnn_lp_layout_for refuses, negative forced sizes or entries without
 * a row, a missing or misaligned buffer, an arena shorter than arena_bytes or not 256-byte aligned, a threshold that is not finite;
 * GCNN_E_UNSUPPORTED for more than 4,096 cuts, or more than 2^24 state rows, columns or forced rows. */
#define GCNN_LP_COLLECT_OUTPUTS 14
enum { GCNN_LP_COLLECT_CONS_FEATS = 0, GCNN_LP_COLLECT_CONS_EDGE_INDS, GCNN_LP_COLLECT_CONS_EDGE_FEATS, GCNN_LP_COLLECT_VAR_FEATS,
       GCNN_LP_COLLECT_CUT_FEATS, GCNN_LP_COLLECT_CUT_EDGE_INDS, GCNN_LP_COLLECT_CUT_EDGE_FEATS, GCNN_LP_COLLECT_CUT_INDEX,
       GCNN_LP_COLLECT_LP_FLAGS, GCNN_LP_COLLECT_HYBRID_QUALITY, GCNN_LP_COLLECT_FEATURES, GCNN_LP_COLLECT_ORDER,
       GCNN_LP_COLLECT_N_KEPT, GCNN_LP_COLLECT_HYBRID_FLAGS };
typedef struct gcnn_lp_collect_layout {
    size_t in_bytes, snap_off[GCNN_LP_ARRAYS], quality_off, forced_off[3], table_off, table_bytes;
    size_t out_bytes, out_off[GCNN_LP_COLLECT_OUTPUTS];
    size_t arena_bytes, out_dev_off, rows_off[3], ws_off, lp_scratch_off, hyb_scratch_off;   /* internal carving of the arena (the upload lies at 0) */
    size_t entry_snap[GCNN_HYBRID_ARRAYS];
} gcnn_lp_collect_layout;
int gcnn_lp_collect_layout_for(const gcnn_lp_dims* dims, int32_t n_forced, int32_t n_forced_entries,
                               gcnn_lp_collect_layout* layout /* host */);
int gcnn_lp_collect(const gcnn_lp_dims* dims, int32_t n_forced, int32_t n_forced_entries, void* host_in, void* host_out, void* arena,
                    size_t arena_bytes, double p_max, double p_max_ub, void* stream);

/* ---- host states of several models in one call: the task farm as the reference fills it (model_evaluator.py:211-219) --------------
 * The evaluators' queue runs `seed` innermost, so the states that wait at a scoring server belong to DIFFERENT models.
 * gcnn_infer_models is gcnn_infer_batch's contract for 1..GCNN_IBATCH_MAX states of 1..GCNN_GROUP_MAX models: model_of_state[s] in
 * 0..n_models-1, NON-DECREASING (a model's states are contiguous; the caller sorts) and without gaps (a model without a state is
 * refused); params[m] (host array of device pointers; two entries may be equal).  Two host->device copies (the states; the launch
 * tables of the grouped forward passes), one device->host copy, nothing synchronised, nothing allocated.
 *
 * host_in / host_out: gcnn_infer_batch's, at layout.u.in_off / out_off, with two differences.  in_off[0], the table, has
 * GCNN_MBATCH_TABLE_WORDS int32: gcnn_infer_batch's columns, then n_models, the first state of every model (entry n_models =
 * n_states) from word +1, and from word +16 the model of every state; gcnn_infer_models_fill_table writes it.  in_off[1], the block
 * the caller keeps zero up to in_off[2], is larger (one closing by-left offset per model).  State s still lies at the union's
 * c/v/k/e1/e2_off[s], and its results at k_off[s].
 * host_staging: pinned, 16-byte aligned, layout.table_bytes bytes (as gcnn_group_forward takes it); the device table lives in the
 * arena.
 * Device work: one index pass over all states (ids relative to the state's model), one stable radix sort of the union's constraint
 * edges by union variable id, one launch that splits its offsets per model, the models' forward passes as a group (one launch per
 * distinct kernel and stage, each model on the sub-union of its own states, with the bits gcnn_infer_batch gives for those states
 * alone), one ranking launch or one selection launch pair over all states.
 * Returned before anything is enqueued: what gcnn_infer_batch returns; GCNN_E_BADARG for n_models outside 1..GCNN_GROUP_MAX, a
 * model_of_state that decreases, skips a model, does not start at 0 or does not end at n_models-1, a missing buffer or an arena
 * shorter than layout.u.arena_bytes; GCNN_E_UNSUPPORTED for a forward pass the group recorder cannot take. */
#define GCNN_MBATCH_TABLE_WORDS (GCNN_IBATCH_TABLE_COLS * GCNN_IBATCH_TABLE_STRIDE + 16 + GCNN_IBATCH_MAX)
typedef struct gcnn_mbatch_layout {
    gcnn_ibatch_layout u;                          /* the union: sizes, upload, download, arena (dev_off: internal) */
    int32_t n_models, first_state[GCNN_GROUP_MAX + 1];
    gcnn_dims model[GCNN_GROUP_MAX];               /* the sizes of every model's sub-union */
    size_t ws_off[GCNN_GROUP_MAX], table_off;      /* internal: the models' forward workspaces and the launch tables in the arena */
    size_t table_bytes;                            /* host_staging holds this much */
} gcnn_mbatch_layout;
int gcnn_infer_models_layout_for(int32_t n_states, const gcnn_dims* dims /* host [n_states] */, const int32_t* n_forced,
                                 const int32_t* n_forced_entries, int32_t mode, int32_t n_models,
                                 const int32_t* model_of_state /* host [n_states] */, gcnn_mbatch_layout* layout /* host */);
/* table: host_in + u.in_off[0] (host), GCNN_MBATCH_TABLE_WORDS int32.  No device work. */
int gcnn_infer_models_fill_table(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                                 int32_t n_models, const int32_t* model_of_state, int32_t* table /* host */);
int gcnn_infer_models(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                      int32_t mode, int32_t n_models, const int32_t* model_of_state, const float* const* params /* host [n_models] */,
                      const void* host_in, void* host_out, void* arena, size_t arena_bytes, void* host_staging, double p_max,
                      double p_max_ub, void* stream);

/* ---- LP snapshots of several models in one call: gcnn_infer_models in front of which the device builds every state -----------------
 * The same farm with workers that send the raw LP (no get_state in the worker): the snapshots that wait belong to DIFFERENT models.
 * gcnn_lp_models is gcnn_lp_batch's contract for 1..GCNN_IBATCH_MAX snapshots of 1..GCNN_GROUP_MAX models, with the two model
 * arguments of gcnn_infer_models: model_of_snapshot[s] under model_of_state's rules (non-decreasing from 0, no gaps; a model without
 * a snapshot is refused), params[m] and host_staging as there.  No kernel of its own: the host half of gcnn_infer_models (nothing
 * enqueued), ONE upload, gcnn_lp_batch's two builder launches -- they leave state s exactly where gcnn_infer_models' upload would
 * have put it and clear that call's zero block --, then gcnn_infer_models' device work unchanged (index pass, by-variable sort and
 * its split per model, the second upload: the launch tables, the forward passes as a group, one ranking launch or one selection
 * launch pair), ONE download.  Every snapshot's state has the bits gcnn_lp_state gives it alone, its results the bits gcnn_lp_batch
 * gives for its own model's snapshots alone.
 *
 * layout.models: gcnn_infer_models' layout for the built states' sizes (u.in_off[1] the zero block, u.in_off[2..8] the seven arrays,
 *   inside the arena; nothing of it is uploaded; table_bytes: what host_staging holds).  layout.lp: every field as in
 *   gcnn_lp_batch_layout, with lp.state == models.u.
 * host_in (pinned, lp.in_bytes): [0, lp.table_bytes) the tables -- gcnn_lp_models_fill_table writes them: gcnn_infer_models' table
 *   (GCNN_MBATCH_TABLE_WORDS int32), then gcnn_lp_batch's descriptor part; the snapshots at lp.snap_base[s], the forced rows at
 *   lp.forced_off, as in gcnn_lp_batch.
 * host_out (pinned, lp.out_bytes): lp.out_off[0..5] as gcnn_lp_batch's: scores, order, n_kept, flags [n][4], LP flags [n][4],
 *   cut_index.  Flags mean what they mean there; a flagged snapshot changes no other snapshot's results.
 * Returned before anything is enqueued: whatever gcnn_lp_batch or gcnn_infer_models returns before enqueueing (GCNN_E_BADARG for n
 * outside 1..GCNN_IBATCH_MAX, a gcnn_lp_dims gcnn_lp_layout_for refuses, n_models outside 1..GCNN_GROUP_MAX, a model_of_snapshot that
 * decreases, skips a model or leaves one without a snapshot, thresholds, buffers; GCNN_E_UNSUPPORTED for a union past 2^24 rows or 2^30
 * edges, edges with nothing to point at, and a forward pass the group recorder cannot take). */
typedef struct gcnn_lp_models_layout {
    gcnn_mbatch_layout models;
    gcnn_lp_batch_layout lp;
} gcnn_lp_models_layout;
int gcnn_lp_models_layout_for(int32_t n, const gcnn_lp_dims* dims /* host [n] */, const int32_t* n_forced,
                              const int32_t* n_forced_entries, int32_t mode, int32_t n_models,
                              const int32_t* model_of_snapshot /* host [n] */, gcnn_lp_models_layout* layout /* host */);
/* table: host_in (host), lp.table_bytes bytes.  No device work. */
int gcnn_lp_models_fill_table(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                              int32_t mode, int32_t n_models, const int32_t* model_of_snapshot, void* table /* host */);
int gcnn_lp_models(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int32_t mode,
                   int32_t n_models, const int32_t* model_of_snapshot, const float* const* params /* host [n_models] */,
                   const void* host_in, void* host_out, void* arena, size_t arena_bytes, void* host_staging, double p_max,
                   double p_max_ub, void* stream);

/* ---- an LP that stays on the device across separation rounds ------------------------------------------------------------------------
 * A solver calls its cut selector once per separation round on the same LP: the rows of round t + 1 are the rows of round t plus the
 * selected cuts; what changes is the solve (row_dual, row_basis, the columns' bounds, basis, values and reduced costs) and the
 * candidate cuts.  Of what gcnn_lp_state derives from the rows only is_tight and dual depend on the solve.  So the caller keeps, in
 * device memory of its own (the library allocates nothing): the raw rows (row_ptr, row_col, row_val, row_lhs, row_rhs), col_type,
 * col_obj, the last given col_lb / col_ub / col_primal / col_primal_avg, and the `derived` block gcnn_lp_rows_build writes from them:
 *   off[0] cons_feats [C,4] f32 with columns 0 and 2 final and 1 and 3 zero | off[1] cons_edge_inds [2,E1] i32 | off[2]
 *   cons_edge_feats [E1] f32 -- values and places exactly gcnn_lp_state's -- | off[3] row_place [R][2] i32: the state row of an LP row's
 *   lhs side and of its rhs side, -1 where that side is not finite | off[4] row_scale [R] f64: norm * obj_norm, the dual's divisor |
 *   off[5] flags [4] i32: gcnn_lp_state's flag words for the rows (any set: the block is NOT valid) | off[6] scratch.
 * gcnn_lp_rows_build (two launches, nothing synchronised) runs at open and after every append of rows; dims: n_rows, n_cols, row_nnz,
 * n_state_rows, n_state_edges and the scalars (the cut fields are not read).  The two CSR orders of the constraint edges then come
 * from gcnn_graph_build on off[1], off[2].
 * A round (gcnn_lp_round, gcnn_lp_round_select): ONE upload of host_in (pinned, in_bytes) -- in_off: header (word 0 = present) |
 * row_dual | row_basis | col_basis | col_lp | col_redcost | col_lb | col_ub | col_primal | col_primal_avg (each of the four only when
 * its GCNN_LPR_* bit of `present` is set: it is then also copied into the resident buffer; else the resident buffer is read) |
 * cut_ptr | cut_col | cut_val | cut_lhs | cut_rhs, then forced_off as in gcnn_infer_select -- two launches that write is_tight and
 * dual into cons_feats at row_place and build the variable and cut parts of the state in the arena (no pass touches a row entry),
 * gcnn_forward's launches on the resident constraint graph and the round's cut graph, the ranking or selection, ONE download of
 * host_out (pinned, out_bytes): out_off as gcnn_lp_layout's (the forward's flag block is always zero here).  dims: the full
 * gcnn_lp_dims of the LP this round stands for.  The result has the bits of gcnn_lp_state / gcnn_lp_infer / gcnn_lp_infer_select on the
 * snapshot assembled from the resident rows and the round.  There is no variable limit.  want_order: 1 ranking (at most 4,096
 * cuts), 0 scores only, -1 the state only (no forward pass: the state's variable and cut parts stay at dev_off[1..5] of the arena).
 * Returned before anything is enqueued: GCNN_E_BADARG (dims, present, pointers, thresholds, a short or misaligned arena, edges with
 * nothing to point at) and GCNN_E_UNSUPPORTED (more than 2^24 state rows, columns or cuts; a selection or ranking of more than
 * 4,096 cuts). */
#define GCNN_LPR_LB 1
#define GCNN_LPR_UB 2
#define GCNN_LPR_PRIMAL 4
#define GCNN_LPR_PRIMAL_AVG 8
#define GCNN_LPR_DERIVED 7
#define GCNN_LPR_ARRAYS 15
#define GCNN_LPR_BLOCKS 11
typedef struct gcnn_lp_rows_layout {
    size_t bytes, off[GCNN_LPR_DERIVED];   /* of the derived block; every offset a multiple of 256 */
} gcnn_lp_rows_layout;
int gcnn_lp_rows_layout_for(const gcnn_lp_dims* dims, gcnn_lp_rows_layout* layout /* host */);
int gcnn_lp_rows_build(const gcnn_lp_dims* dims, const int32_t* row_ptr, const int32_t* row_col, const double* row_val,
                       const double* row_lhs, const double* row_rhs, const double* col_obj, void* derived /* device, 256-byte aligned */,
                       size_t derived_bytes, void* stream);
typedef struct gcnn_lp_resident {          /* device pointers */
    const int32_t* row_place; const double* row_scale; float* cons_feats;
    const int8_t* col_type; const double* col_obj;
    double *col_lb, *col_ub, *col_primal, *col_primal_avg;   /* [V] each: the last given values */
    gcnn_graph cons_graph;                 /* gcnn_graph_build of the derived edge list, C left nodes */
} gcnn_lp_resident;
typedef struct gcnn_lp_round_layout {
    size_t in_bytes, in_off[GCNN_LPR_ARRAYS], forced_off[3];
    size_t out_bytes, out_off[6];
    /* the arena: upload | var_feats [V,14] | cut_feats [K,6] | cut_edge_inds [2,E2] | cut_edge_feats [E2] | cut l_ptr [K+1] | output
     * block | forward workspace | the forward's flag block | scratch | selection workspace */
    size_t arena_bytes, dev_off[GCNN_LPR_BLOCKS];
} gcnn_lp_round_layout;
int gcnn_lp_round_layout_for(const gcnn_lp_dims* dims, int32_t present, int32_t n_forced /* < 0: gcnn_lp_round */,
                             int32_t n_forced_entries, gcnn_lp_round_layout* layout /* host */);
int gcnn_lp_round(const gcnn_lp_dims* dims, int32_t present, const gcnn_lp_resident* resident /* host */, const float* params,
                  const void* host_in, void* host_out, void* arena, size_t arena_bytes, int32_t want_order, void* stream);
int gcnn_lp_round_select(const gcnn_lp_dims* dims, int32_t present, int32_t n_forced, int32_t n_forced_entries,
                         const gcnn_lp_resident* resident /* host */, const float* params, const void* host_in, void* host_out,
                         void* arena, size_t arena_bytes, double p_max, double p_max_ub, void* stream);

/* ---- rows appended to a resident LP without deriving the resident rows again ---------------------------------------------------------
 * What gcnn_lp_rows_build and gcnn_graph_build derive from a row is local to that row but its place: the state lists the lhs sides
 * first, so appended lhs rows move every rhs row.  An append therefore copies, shifts and merges the resident arrays and derives only
 * the new rows -- through the same functions as the rebuild, so the result has its bits.  The caller holds TWO sets of derived
 * arrays (gcnn_lp_rows_set: what the rebuild's derived block and graph hold, as separate arrays; edge_col / edge_coef are the graph's
 * l_oth / l_coef).  An append reads `src` and writes `dst`, which must hold the sizes after the append; src is not written, so a
 * rejected block costs nothing to undo.  block: its rows, raw entries, state rows and state edges, how many of the state rows and
 * edges are lhs sides, and the same two counts of the resident state.  dims: the resident LP BEFORE the append.
 * gcnn_lp_rows_append: the raw row arrays already hold the block behind the resident rows (row_ptr absolute); one fill of the count
 * tables and four launches (k_lpa_stats, k_lpa_scan, k_lpa_move, k_lpa_order); the four flag words (gcnn_lp_state's; any set: dst is
 * NOT valid) go to the device address `flags`; nothing is synchronised.
 * gcnn_lp_round_append: the append inside the call of the round that follows it.  ONE upload of host_in (in_bytes): the block at
 * block_off[0..4] -- row_ptr [n_rows + 1] from 0, row_col, row_val, row_lhs, row_rhs, unpadded -- then, at block_bytes (a multiple of 256), the round's upload as
 * gcnn_lp_round_layout_for lays it out for the dims AFTER the append (row_dual and row_basis cover the new rows), forced rows
 * included.  The append's launches also copy the block behind the resident raw rows (whose buffers must have the room); then exactly
 * what gcnn_lp_round / gcnn_lp_round_select enqueue on `resident`, which points at dst; ONE download of out_bytes: the round's, then the
 * append's four flag words at flags_off.  n_forced >= 0: a selection (want_order is not read); else want_order as gcnn_lp_round's.
 * The arena: the upload | at round_off the round's arena | at scratch_off the append's scratch.  Returned before anything is
 * enqueued: GCNN_E_BADARG, GCNN_E_WORKSPACE and the round's GCNN_E_UNSUPPORTED limits on the dims after the append. */
typedef struct gcnn_lp_append_dims {
    int32_t n_rows, row_nnz, n_state_rows, n_state_edges;   /* the block */
    int32_t n_lhs_rows, n_lhs_edges;                          /* of them, lhs sides */
    int32_t res_lhs_rows, res_lhs_edges;                      /* lhs sides of the resident state */
} gcnn_lp_append_dims;
typedef struct gcnn_lp_rows_set {          /* device pointers */
    float* cons_feats; int32_t* edge_row; int32_t* edge_col; float* edge_coef;
    int32_t* l_ptr; int32_t* v_ptr; int32_t* v_oth; float* v_coef;
    int32_t* row_place; double* row_scale;
} gcnn_lp_rows_set;
typedef struct gcnn_lp_append_layout {
    size_t block_bytes, block_off[5], in_bytes;
    size_t out_bytes, flags_off;
    size_t scratch_bytes;                  /* what gcnn_lp_rows_append needs */
    size_t arena_bytes, round_off, scratch_off;
    gcnn_lp_round_layout round;            /* offsets relative to block_bytes (upload), 0 (download) and round_off (arena) */
} gcnn_lp_append_layout;
int gcnn_lp_append_layout_for(const gcnn_lp_dims* dims, const gcnn_lp_append_dims* block, int32_t present, int32_t n_forced,
                              int32_t n_forced_entries, gcnn_lp_append_layout* layout /* host */);
int gcnn_lp_rows_append(const gcnn_lp_dims* dims, const gcnn_lp_append_dims* block, const int32_t* row_ptr, const int32_t* row_col,
                        const double* row_val, const double* row_lhs, const double* row_rhs, const double* col_obj,
                        const gcnn_lp_rows_set* src /* host */, const gcnn_lp_rows_set* dst /* host */, void* scratch, size_t scratch_bytes,
                        int32_t* flags /* device [4] */, void* stream);
int gcnn_lp_round_append(const gcnn_lp_dims* dims, const gcnn_lp_append_dims* block, int32_t present, int32_t n_forced,
                         int32_t n_forced_entries, int32_t* row_ptr, int32_t* row_col, double* row_val, double* row_lhs, double* row_rhs,
                         const gcnn_lp_rows_set* src /* host */, const gcnn_lp_rows_set* dst /* host */,
                         const gcnn_lp_resident* resident /* host; on dst */, const float* params, const void* host_in, void* host_out,
                         void* arena, size_t arena_bytes, int32_t want_order, double p_max, double p_max_ub, void* stream);

/* ---- rows removed from a resident LP without deriving anything again -------------------------------------------------------------------
 * Between two separation rounds a solver also cleans its LP: rows that have been slack for a while leave again.  Removal is the
 * mirror image of the append: nothing is derived and no floating-point value is computed; every kept value is copied and every kept
 * index renumbered by a monotone map, so both CSR orders stay stable: rows [kept lhs | kept rhs], by-left edges likewise, per
 * variable the kept entries of its old segment in their old order, v_ptr = old v_ptr - exclusive prefix of the removed counts;
 * row_place, row_scale, l_ptr, the 16-byte cons_feats rows and the five raw arrays (row_ptr re-based) are compacted by the same
 * launches.  Everything goes out of place: the removal reads `src` and the raw rows and writes `dst` and a SECOND set of raw
 * buffers (out_*), so a rejected call costs nothing to undo; no source may overlap a destination.
 * removed: what the host counted of the removed rows -- rows, raw entries, state rows, state edges, how many of the state rows and
 * edges are lhs sides -- and the lhs rows and entries of the resident state.  dims: the resident LP BEFORE the edit.  list: the removed
 * LP rows, ascending, int32.
 * gcnn_lp_rows_remove: the removal alone; list on the device; one fill of the removed counters and three launches (k_lpd_mark,
 * k_lpd_rows, k_lpd_vars); the four flag words (word 3: the device's totals differ from the host's; any set: dst is NOT valid) go
 * to the device address `flags`; nothing is synchronised.
 * gcnn_lp_round_remove: the removal -- and, with `block`, an append behind it -- inside the call of the round that follows.  ONE
 * upload of host_in (in_bytes): the list (list_bytes, a multiple of 256), then exactly gcnn_lp_round's upload, or with a block
 * gcnn_lp_round_append's, for the dims AFTER the edit (block_off absolute, round.in_off relative to list_bytes + block_bytes).
 * The removal's launches; with a block exactly gcnn_lp_round_append's append launches from `transit` (what the removal wrote; never
 * src or dst) into dst, its rows copied behind the rows of out_* (whose buffers must have the room); then exactly what gcnn_lp_round /
 * gcnn_lp_round_select enqueue on `resident`, which points at dst; ONE download of out_bytes: that call's, then the removal's four
 * flag words at flags_off (with a block the append's at append_flags_off in front of them); no host wait in between.  block's
 * res_lhs_* are the lhs counts after the removal.  The arena: the upload | at round_off the round's arena | the append's scratch at
 * append_scratch_off | the removal's scratch at scratch_off.  The library allocates nothing.
 * Returned before anything is enqueued: GCNN_E_BADARG (counts that cannot be: negative, more removed than resident, lhs counts above
 * the totals, nothing left after the whole edit; a missing pointer; a misaligned cons_feats; a source set, raw buffer or transit set
 * that overlaps a destination; a short or misaligned arena; thresholds that are not finite), GCNN_E_WORKSPACE (a short scratch) and
 * GCNN_E_UNSUPPORTED (the round's limits on the dims after the edit).  Not part of gcnn_lp_rounds; gcnn_lp_rounds_edit (below) takes a
 * member with a removal and gives it what this call gives. */
typedef struct gcnn_lp_remove_dims {
    int32_t n_rows, row_nnz, n_state_rows, n_state_edges;   /* the removed rows */
    int32_t n_lhs_rows, n_lhs_edges;                          /* of them, lhs sides */
    int32_t res_lhs_rows, res_lhs_edges;                      /* lhs sides of the resident state */
} gcnn_lp_remove_dims;
typedef struct gcnn_lp_remove_layout {
    size_t list_bytes;                     /* the list opens the upload */
    size_t block_bytes, block_off[5];      /* with a block: as gcnn_lp_append_layout's, offsets from the upload's start; else 0 */
    size_t in_bytes, out_bytes;
    size_t flags_off, append_flags_off;
    size_t scratch_bytes;                  /* what gcnn_lp_rows_remove needs */
    size_t arena_bytes, round_off, append_scratch_off, scratch_off;
    gcnn_lp_round_layout round;            /* offsets relative to list_bytes + block_bytes (upload), 0 (download) and round_off (arena) */
} gcnn_lp_remove_layout;
int gcnn_lp_remove_layout_for(const gcnn_lp_dims* dims, const gcnn_lp_remove_dims* removed, const gcnn_lp_append_dims* block /* or NULL */,
                              int32_t present, int32_t n_forced, int32_t n_forced_entries, gcnn_lp_remove_layout* layout /* host */);
int gcnn_lp_rows_remove(const gcnn_lp_dims* dims, const gcnn_lp_remove_dims* removed, const int32_t* list /* device */,
                        const int32_t* row_ptr, const int32_t* row_col, const double* row_val, const double* row_lhs, const double* row_rhs,
                        int32_t* out_ptr, int32_t* out_col, double* out_val, double* out_lhs, double* out_rhs,
                        const gcnn_lp_rows_set* src /* host */, const gcnn_lp_rows_set* dst /* host */, void* scratch, size_t scratch_bytes,
                        int32_t* flags /* device [4] */, void* stream);
int gcnn_lp_round_remove(const gcnn_lp_dims* dims, const gcnn_lp_remove_dims* removed, const gcnn_lp_append_dims* block /* or NULL */,
                         int32_t present, int32_t n_forced, int32_t n_forced_entries, const int32_t* row_ptr, const int32_t* row_col,
                         const double* row_val, const double* row_lhs, const double* row_rhs, int32_t* out_ptr, int32_t* out_col,
                         double* out_val, double* out_lhs, double* out_rhs, const gcnn_lp_rows_set* src /* host */,
                         const gcnn_lp_rows_set* transit /* host; with a block */, const gcnn_lp_rows_set* dst /* host */,
                         const gcnn_lp_resident* resident /* host; on dst */, const float* params, const void* host_in, void* host_out,
                         void* arena, size_t arena_bytes, int32_t want_order, double p_max, double p_max_ub, void* stream);

/* ---- rounds of several resident LPs in one call -------------------------------------------------------------------------------------
 * What a scoring server holds when several solver workers each keep an LP resident: one round per session, waiting at the same time.
 * gcnn_lp_rounds serves 1..GCNN_LP_ROUNDS_MAX of them with ONE upload, ONE upload of launch tables, at most ONE fill, one launch per
 * stage and distinct kernel, and ONE download -- the number of enqueued operations does not depend on n for same-shaped members.
 * Member i brings what its solo call brings: dims, present, n_forced / n_forced_entries, resident, params and, with has_append, the
 * arguments of gcnn_lp_round_append (dims then describe the LP BEFORE the append, resident points at dst).  mode (GCNN_IBATCH_SCORES /
 * _RANK / _SELECT), p_max and p_max_ub hold for every member; n_forced is >= 0 for every member in selection mode and -1 otherwise.
 * Each member's work is its solo call's, recorded instead of launched (gcnn_group_forward's mechanism): every launch of the solo
 * round and append has a group twin that runs the solo body with the member's arguments and its solo (block, blocks) pair.  So the
 * member's download block (scores | order | flags | n_kept | LP flags | cut_index | the append's flags, exactly the solo out_off /
 * flags_off, at out_off[i] of the call's download) and everything it leaves resident (cons_feats, the optional column buffers, the
 * raw rows and dst of an append) have the bits of gcnn_lp_round / gcnn_lp_round_select / gcnn_lp_round_append on that member alone.
 * The appends' launches form a phase of their own in front, so that the rounds share their stages whether or not a member appends.
 * A member whose state has no constraint rows, columns or cuts runs its round's solo launches inside the call, behind the others.
 * The arena (the caller's; the library allocates nothing): all uploads, member after member at in_off[i] (each the solo upload: the
 * append block, the round, the forced rows; in_size[i] = the solo in_bytes rounded up to 256) | per member at arena_off[i] the solo
 * arena (gcnn_lp_round_layout_for, or gcnn_lp_append_layout_for's from round_off on, at member_round_off[i]; the append's scratch at
 * scratch_off[i]) | the appends' count tables, contiguous (the one fill) | all download blocks at out_off[i] from out_base on | the
 * launch tables at table_off.  host_staging: pinned, table_bytes.  host_in: in_bytes, laid out as the arena's front; host_out:
 * out_bytes, as the arena from out_base on.
 * Returned before anything is enqueued: GCNN_E_BADARG (n outside 1..GCNN_LP_ROUNDS_MAX, a missing pointer, anything a member's solo
 * call refuses, a short or misaligned arena, thresholds that are not finite, a member's writable memory -- cons_feats, the
 * optional column buffers, the raw rows and dst of an append -- overlapping any memory of another member, which covers one session
 * given twice), GCNN_E_WORKSPACE (a short table) and GCNN_E_UNSUPPORTED (the solo limits; more than 4,096 cuts in an ordering mode;
 * a member whose launches the recorder cannot take). */
#define GCNN_LP_ROUNDS_MAX GCNN_GROUP_MAX
typedef struct gcnn_lp_rounds_member {
    gcnn_lp_dims dims;
    int32_t present, n_forced, n_forced_entries;
    int32_t has_append;
    gcnn_lp_append_dims block;                                              /* has_append */
    int32_t* row_ptr; int32_t* row_col; double* row_val; double* row_lhs; double* row_rhs;   /* has_append: the raw rows (device) */
    const gcnn_lp_rows_set* src; const gcnn_lp_rows_set* dst;             /* has_append (host) */
    const gcnn_lp_resident* resident;                                       /* host */
    const float* params;
} gcnn_lp_rounds_member;
typedef struct gcnn_lp_rounds_layout {
    int32_t n, mode;
    size_t in_bytes, in_off[GCNN_LP_ROUNDS_MAX], in_size[GCNN_LP_ROUNDS_MAX];
    size_t arena_off[GCNN_LP_ROUNDS_MAX], member_round_off[GCNN_LP_ROUNDS_MAX], scratch_off[GCNN_LP_ROUNDS_MAX];
    size_t counts_base, counts_bytes, counts_off[GCNN_LP_ROUNDS_MAX];
    size_t out_base, out_bytes, out_off[GCNN_LP_ROUNDS_MAX], out_size[GCNN_LP_ROUNDS_MAX];   /* out_off: relative to out_base */
    size_t table_off, table_bytes;
    size_t arena_bytes;
} gcnn_lp_rounds_layout;
int gcnn_lp_rounds_layout_for(int32_t n, const gcnn_lp_rounds_member* members /* host; only the sizes are read */, int32_t mode,
                              gcnn_lp_rounds_layout* layout /* host */);
int gcnn_lp_rounds(int32_t n, const gcnn_lp_rounds_member* members /* host */, int32_t mode, const void* host_in, void* host_out,
                   void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream);

/* ---- rounds of several resident LPs in one call, with removals ------------------------------------------------------------------------
 * gcnn_lp_rounds with an optional removal per member: what the server holds when the workers' solvers clean their LPs between rounds.
 * A member holds what gcnn_lp_rounds_member holds, in the same order; with has_remove it adds the remaining arguments of
 * gcnn_lp_round_remove: `removed`, the five out_* raw buffers and, needed only with has_append, `transit`.  dims then describe the LP
 * BEFORE any edit, row_* are the raw SOURCE (read), src is read by the removal, resident points at dst, and block's res_lhs_* are the
 * counts after the removal, exactly as in the solo call.  A member with has_remove = 0 means what it means in gcnn_lp_rounds.
 * The contract is gcnn_lp_rounds', extended: every member's download block (the solo call's, the append's flag words at the solo
 * append_flags_off / flags_off, the removal's four at the solo flags_off) and everything the member leaves resident (cons_feats, the
 * optional column buffers, the out_* raw rows, dst, the transit set) have the bits of the member's solo call on that member alone --
 * gcnn_lp_round / _select, gcnn_lp_round_append or gcnn_lp_round_remove, as its edits require.  The removal's three launches have group
 * twins like every other launch (k_lpes_mark, k_lpes_rows, k_lpes_vars run the bodies of k_lpd_mark, k_lpd_rows, k_lpd_vars with the
 * member's arguments and its solo block index).
 * Three phases, each recorded and planned on its own: the removals (at most 3 stages), the appends (at most 4) reading what the
 * removals wrote, the rounds -- so the members' round launches share their stages whatever edits a member carries.  For n same-shaped
 * members the launches are those of one solo call of the same kind whatever n is: 11 plain, 14 with a removal, 15 with an append, 18
 * with both.  Enqueued: ONE upload of all members' uploads, ONE of the launch tables, at most ONE fill (the removals' counters and the
 * appends' count tables lie side by side: counts_base, counts_bytes), the launches, ONE download; no host wait, no device-to-device
 * copy.  A member whose state after the edits has no constraint rows, columns or cuts: its edits ride in the edit phases, its
 * round's solo launches run inside the call, behind the others.
 * The arena: all uploads, member after member at in_off[i] (each the solo upload -- the list, the block, the round, the forced rows, as
 * gcnn_lp_remove_layout_for / gcnn_lp_append_layout_for / gcnn_lp_round_layout_for lay it out; in_size[i] = the solo in_bytes rounded up
 * to 256) | per member at arena_off[i] the solo arena (the round's at member_round_off[i], the append's scratch at scratch_off[i], the
 * removal's at remove_scratch_off[i]; its counters are not used there) | the fill region: per member the removal's counters at
 * remove_counts_off[i], then the append's count tables at counts_off[i] | all download blocks at out_off[i] from out_base on | the
 * launch tables at table_off (sized for 3 + 4 + 16 stages a member).  host_staging: pinned, table_bytes.
 * Returned before anything is enqueued: what gcnn_lp_rounds returns, on the dims each check applies to; what gcnn_lp_round_remove
 * refuses of a member (its counts, a missing out_* or transit, a transit set equal to src or dst, out_* over the raw source); across
 * members the overlap rule extended by what a removing member writes (out_*, the transit set, dst) and reads (src, the raw source). */
typedef struct gcnn_lp_rounds_edit_member {
    gcnn_lp_dims dims;
    int32_t present, n_forced, n_forced_entries;
    int32_t has_append;
    gcnn_lp_append_dims block;                                              /* has_append */
    int32_t* row_ptr; int32_t* row_col; double* row_val; double* row_lhs; double* row_rhs;   /* an edit: the raw rows (device) */
    const gcnn_lp_rows_set* src; const gcnn_lp_rows_set* dst;             /* an edit (host) */
    const gcnn_lp_resident* resident;                                       /* host */
    const float* params;
    int32_t has_remove, reserved;
    gcnn_lp_remove_dims removed;                                            /* has_remove */
    int32_t* out_ptr; int32_t* out_col; double* out_val; double* out_lhs; double* out_rhs;   /* has_remove: the second raw set (device) */
    const gcnn_lp_rows_set* transit;                                        /* has_remove and has_append (host) */
} gcnn_lp_rounds_edit_member;
typedef struct gcnn_lp_rounds_edit_layout {
    int32_t n, mode;
    size_t in_bytes, in_off[GCNN_LP_ROUNDS_MAX], in_size[GCNN_LP_ROUNDS_MAX];
    size_t arena_off[GCNN_LP_ROUNDS_MAX], member_round_off[GCNN_LP_ROUNDS_MAX], scratch_off[GCNN_LP_ROUNDS_MAX];
    size_t remove_scratch_off[GCNN_LP_ROUNDS_MAX];
    size_t counts_base, counts_bytes, counts_off[GCNN_LP_ROUNDS_MAX], remove_counts_off[GCNN_LP_ROUNDS_MAX];
    size_t out_base, out_bytes, out_off[GCNN_LP_ROUNDS_MAX], out_size[GCNN_LP_ROUNDS_MAX];   /* out_off: relative to out_base */
    size_t table_off, table_bytes;
    size_t arena_bytes;
} gcnn_lp_rounds_edit_layout;
int gcnn_lp_rounds_edit_layout_for(int32_t n, const gcnn_lp_rounds_edit_member* members /* host; only the sizes are read */, int32_t mode,
                                   gcnn_lp_rounds_edit_layout* layout /* host */);
int gcnn_lp_rounds_edit(int32_t n, const gcnn_lp_rounds_edit_member* members /* host */, int32_t mode, const void* host_in, void* host_out,
                        void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream);

/* ---- ensembles: ONE state scored by several models, their mean ranked or selected once -----------------------------------------------
 * The reference trains five seeds per problem (train_models, model_trainer.py:38-49); its selector plugin ranks and filters by ONE
 * quality vector (model_evaluator.py:82-154).  These entry points let 1..GCNN_GROUP_MAX models score the same round and hand the
 * plugin the mean of their predicted bound improvements.  For members m = 0..M-1 in the caller's order and a state with K cuts:
 *   member[m][k]  model m's score of cut k: the bits gcnn_infer_models gives for that state and that model;
 *   mean[k]       acc = member[0][k]; acc = acc + member[m][k] for m = 1..M-1 in that order; acc / float(M) -- every step fp32,
 *                 rounded to nearest, nothing contracted: a float32 loop on the host gives the same bits.  M == 1: mean ==
 *                 member[0] bit for bit.  A NaN in any member gives a NaN mean.
 * gcnn_ensemble_mean is that combination alone (model_evaluator.py:82-154 reads its result, model_trainer.py:38-49 supplies its
 * inputs): member_scores is a HOST array of n_models DEVICE pointers to [n] floats, mean [n] is device memory; one launch on
 * `stream`, none for n == 0.  GCNN_E_BADARG for n_models outside 1..GCNN_GROUP_MAX, n < 0, or a null pointer with n > 0. */
int gcnn_ensemble_mean(const float* const* member_scores /* host [n_models] of device pointers */, int32_t n_models, int32_t n,
                       float* mean /* device [n] */, void* stream);
/* gcnn_infer_ensemble (model_evaluator.py:82-154 for the models of model_trainer.py:38-49): gcnn_infer_batch's contract for ONE host
 * state and n_models models.  mode: GCNN_IBATCH_SCORES / _RANK / _SELECT.  host_in (pinned): gcnn_infer_batch's upload of one state
 * at layout.u.in_off (the table written by gcnn_infer_batch_fill_table(1, ...), the zero block, the seven arrays with STATE-LOCAL
 * ids, the forced rows in selection mode) -- the state goes up ONCE, whatever n_models is.  params: host array of n_models device
 * pointers, all different.  host_staging: pinned, 16-byte aligned, layout.table_bytes bytes (the launch tables of the grouped
 * forward passes; the second host->device copy).
 * Device work: the index pass and the by-variable sort of the one state (ONE graph plan), the n_models forward passes as one group
 * (one launch per distinct kernel and stage; every member reads the same feature arrays and the same two graphs and has its own
 * parameters, workspace and score row), the mean, then gcnn_infer_batch's ranking of, or gcnn_select_cuts' filter over, the mean.
 * host_out (pinned, layout.u.out_bytes), ONE device->host copy: u.out_off[0] mean [K], u.out_off[1] order [K] int32 (RANK: the
 * descending stable ranking of the mean, NaN as -inf; SELECT: as gcnn_select_cuts), u.out_off[2] n_kept int32 (SELECT), u.out_off[3]
 * the four flags of gcnn_infer_batch, and at member_off + m * member_stride member[m] [K].  A flag set => nothing else is valid.
 * The arena holds n_models forward workspaces.  Returned before anything is enqueued: GCNN_E_BADARG for n_models outside
 * 1..GCNN_GROUP_MAX, a negative size, an unknown mode, a missing buffer, a short or misaligned arena, a threshold that is not
 * finite; GCNN_E_UNSUPPORTED for more than 32,768 variables, for more than 4,096 cuts in RANK / SELECT, for edges with nothing to
 * point at and for a forward pass the group recorder cannot take: the caller takes the general path (gcnn_graph_build,
 * gcnn_group_forward, gcnn_ensemble_mean, gcnn_select_cuts), which gives the same bits. */
typedef struct gcnn_ensemble_layout {
    gcnn_ibatch_layout u;                          /* the one state's union: upload, download, arena (dev_off: internal) */
    int32_t n_models, reserved;
    size_t member_off, member_stride;              /* host_out: member m's scores at member_off + m * member_stride */
    size_t ws_off[GCNN_GROUP_MAX], table_off;      /* internal: the members' forward workspaces and the launch tables in the arena */
    size_t table_bytes;                            /* host_staging holds this much */
} gcnn_ensemble_layout;
int gcnn_infer_ensemble_layout_for(const gcnn_dims* dims, int32_t n_forced, int32_t n_forced_entries, int32_t mode, int32_t n_models,
                                   gcnn_ensemble_layout* layout /* host */);
int gcnn_infer_ensemble(const gcnn_dims* dims, int32_t n_forced, int32_t n_forced_entries, int32_t mode, int32_t n_models,
                        const float* const* params /* host [n_models] */, const void* host_in, void* host_out, void* arena,
                        size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream);
/* gcnn_lp_ensemble (model_evaluator.py:82-154 for the models of model_trainer.py:38-49): the same from ONE raw LP snapshot --
 * gcnn_lp_batch's contract for one snapshot and n_models models.  ONE upload of the packed snapshot (+ forced rows), gcnn_lp_batch's
 * two builder launches build the state ONCE where gcnn_infer_ensemble's upload would have put it, then that call's device work.
 * layout.ens: gcnn_infer_ensemble's layout for the built state's sizes (nothing of it is uploaded); layout.lp: as in
 * gcnn_lp_batch_layout with lp.state == ens.u.  host_in (pinned, lp.in_bytes, WRITABLE): the call itself writes the tables into
 * [0, lp.table_bytes); the caller packs the snapshot at lp.snap_base[0] + gcnn_lp_layout.snap_off[i] and the forced rows at
 * lp.forced_off.  host_out (pinned, lp.out_bytes): gcnn_infer_ensemble's block (mean, order, n_kept, flags, members at
 * ens.member_off), then lp.out_off[4] the four LP flags and lp.out_off[5] cut_index [K].  Everything is in STATE order.
 * Returned before anything is enqueued: what gcnn_infer_ensemble returns for the built state's sizes, and GCNN_E_BADARG for a
 * gcnn_lp_dims gcnn_lp_layout_for refuses. */
typedef struct gcnn_lp_ensemble_layout {
    gcnn_ensemble_layout ens;
    gcnn_lp_batch_layout lp;
} gcnn_lp_ensemble_layout;
int gcnn_lp_ensemble_layout_for(const gcnn_lp_dims* dims, int32_t n_forced, int32_t n_forced_entries, int32_t mode, int32_t n_models,
                                gcnn_lp_ensemble_layout* layout /* host */);
int gcnn_lp_ensemble(const gcnn_lp_dims* dims, int32_t n_forced, int32_t n_forced_entries, int32_t mode, int32_t n_models,
                     const float* const* params /* host [n_models] */, void* host_in, void* host_out, void* arena, size_t arena_bytes,
                     void* host_staging, double p_max, double p_max_ub, void* stream);

/* ---- ensembles over many states: what waits at a farm's scoring server, scored by ONE ensemble in one call ----------------------------
 * gcnn_infer_ensemble_batch (the evaluators' farm of SCIP workers, model_evaluator.py:157-241, each deploying the five seeds of
 * model_trainer.py:38-49 as an ensemble): gcnn_infer_ensemble for 1..GCNN_IBATCH_MAX host states at once.  dims, n_forced,
 * n_forced_entries, mode, host_in: exactly gcnn_infer_batch's (layout.u is that call's layout for these states: in_bytes, in_off and
 * out_off are the same, byte for byte, whatever n_models is; the table is written by gcnn_infer_batch_fill_table).  params,
 * host_staging: as gcnn_infer_ensemble takes them.  The call writes nothing into host_in.
 * Enqueued, in this order: ONE upload of the states; the index pass; the by-variable stage of the union, ONCE; the launch tables of
 * the group (the second host->device copy); the n_models forward passes over the union as ONE group (the members of an ensemble
 * over a union are still the members of one group, so n_models <= GCNN_GROUP_MAX is the only bound); the mean (gcnn_ensemble_mean's
 * definition); the per-state tail -- RANK: mean and ranking of every state's segment in one launch of its own, SELECT:
 * gcnn_infer_batch's selection over all states, each with its own forced rows; ONE download.
 * host_out (pinned, layout.u.out_bytes): gcnn_infer_batch's block with the mean where the scores were -- u.out_off[0] mean [K_total]
 * (state s at k_off[s]), u.out_off[1] order [K_total] (state-local cut indices), u.out_off[2] n_kept [n_states], u.out_off[3] flags
 * [n_states][4] -- and behind it, at member_off + m * member_stride, member[m] [K_total]: member_stride = the 16-byte multiple that
 * holds 4 * K_total bytes.  member[m]'s bits are those of gcnn_infer_batch for model m on the same states in the same order.  A
 * state with a flag set has no valid results and changes no other state's (gcnn_infer_batch).
 * Returned before anything is enqueued: what gcnn_infer_batch returns for these sizes (n_states outside 1..GCNN_IBATCH_MAX, a negative
 * size, an unknown mode, a union past 2^24 rows or 2^30 edges, edges with nothing to point at, thresholds that are not finite,
 * missing buffers, a short or misaligned arena); GCNN_E_BADARG for n_models outside 1..GCNN_GROUP_MAX, a null params entry and a
 * missing host_staging; GCNN_E_UNSUPPORTED for a state of more than 4,096 cuts in RANK / SELECT and for a forward pass the group
 * recorder cannot take (the caller serves the states one by one).  There is no variable limit. */
int gcnn_infer_ensemble_batch_layout_for(int32_t n_states, const gcnn_dims* dims /* host [n_states] */, const int32_t* n_forced,
                                         const int32_t* n_forced_entries, int32_t mode, int32_t n_models,
                                         gcnn_ensemble_layout* layout /* host */);
int gcnn_infer_ensemble_batch(int32_t n_states, const gcnn_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries,
                              int32_t mode, int32_t n_models, const float* const* params /* host [n_models] */, const void* host_in,
                              void* host_out, void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub,
                              void* stream);
/* gcnn_lp_ensemble_batch (the evaluators' farm, model_evaluator.py:157-241, with the five seeds of model_trainer.py:38-49 as one
 * ensemble): the same from 1..GCNN_IBATCH_MAX raw LP snapshots -- gcnn_lp_batch's contract for n snapshots and n_models models.
 * ONE upload (tables | packed snapshots | forced rows), gcnn_lp_batch's two builder launches build every state ONCE where
 * gcnn_infer_ensemble_batch's upload would have put it, then that call's device work.  layout.ens: gcnn_infer_ensemble_batch's
 * layout for the built states' sizes; layout.lp: as in gcnn_lp_batch_layout with lp.state == ens.u.  host_in (pinned, lp.in_bytes,
 * WRITABLE): the call itself writes the tables into [0, lp.table_bytes), as gcnn_lp_ensemble does; the caller packs snapshot s at
 * lp.snap_base[s] + gcnn_lp_layout.snap_off[i] and the stacked forced rows at lp.forced_off.  host_out (pinned, lp.out_bytes):
 * gcnn_infer_ensemble_batch's block (members at ens.member_off), then lp.out_off[4] the LP flags [n][4] and lp.out_off[5] cut_index
 * [K_total], as gcnn_lp_batch lays them out.  Everything is in STATE order.  Returned before anything is enqueued: what
 * gcnn_infer_ensemble_batch returns for the built states' sizes and what gcnn_lp_batch returns for these snapshots. */
int gcnn_lp_ensemble_batch_layout_for(int32_t n, const gcnn_lp_dims* dims /* host [n] */, const int32_t* n_forced,
                                      const int32_t* n_forced_entries, int32_t mode, int32_t n_models,
                                      gcnn_lp_ensemble_layout* layout /* host */);
int gcnn_lp_ensemble_batch(int32_t n, const gcnn_lp_dims* dims, const int32_t* n_forced, const int32_t* n_forced_entries, int32_t mode,
                           int32_t n_models, const float* const* params /* host [n_models] */, void* host_in, void* host_out,
                           void* arena, size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream);

/* ---- a round of ONE resident LP scored by an ensemble -------------------------------------------------------------------------------
 * gcnn_lp_round_ensemble (model_evaluator.py:82-154 for the models of model_trainer.py:38-49): what gcnn_lp_ensemble gives for the
 * snapshot assembled from the resident rows and this round, without uploading or deriving the rows again.  Nothing in a resident LP
 * belongs to a model.  `round` is the description of one round of one resident LP that gcnn_lp_rounds_edit takes, with its optional
 * removal and optional append (its `params` field is not read); mode: GCNN_IBATCH_SCORES / _RANK / _SELECT, n_forced >= 0 in
 * selection mode and -1 otherwise.  params: host array of n_models device pointers, all different.  host_staging: pinned, 16-byte
 * aligned, table_bytes bytes.
 * Enqueued, in this order: ONE upload of host_in (in_bytes) -- byte for byte the solo call's of this round and these edits
 * (gcnn_lp_round_layout_for / gcnn_lp_append_layout_for / gcnn_lp_remove_layout_for: the list | the block | the round | the forced
 * rows), so it does not depend on n_models; the edits' launches; the round's two state launches, ONCE; the launch tables of the
 * group (the second host->device copy) and the n_models forward passes as one group, one launch per distinct kernel and stage --
 * every member reads the same feature arrays, the resident constraint graph and the round's cut graph, and has its own parameters,
 * forward workspace and score row; the mean (gcnn_ensemble_mean's definition); the solo round's ranking or selection over the mean;
 * ONE download of out_bytes.  No kernel is this call's own.
 * host_out: the solo call's download block with the mean where the scores were -- round.out_off[0] mean [K], [1] order, [3] n_kept,
 * [4] the four LP flags, [5] cut_index, the edits' flag words at append_flags_off / flags_off as in the solo layouts -- then at
 * member_off + m * member_stride member[m] [K]: the bits gcnn_lp_round gives for model m.  Everything the call leaves resident has
 * the bits the solo call of the same round and edits leaves.  A state without constraint rows or columns runs the members' solo
 * launches inside the call; a round without cuts scores nothing and only refreshes the resident columns.
 * The arena: the solo call's arena (solo_arena_bytes; the round's part at round_off, round.dev_off relative to it) | at out_base the
 * download block and the members' rows | the forward workspaces at ws_off[m] | the launch tables at table_off.
 * Returned before anything is enqueued: GCNN_E_BADARG for n_models outside 1..GCNN_GROUP_MAX, a null or repeated entry of params, a
 * missing or misaligned host_staging, an unknown mode, n_forced < 0 in selection mode or >= 0 otherwise, a short or misaligned
 * arena, and everything the solo call of the round refuses; GCNN_E_WORKSPACE for a short table; GCNN_E_UNSUPPORTED for the solo
 * limits (2^24 rows per table, more than 4,096 cuts in RANK / SELECT) and a forward pass the group recorder cannot take.  There is
 * no variable limit. */
typedef struct gcnn_lp_round_ensemble_layout {
    gcnn_lp_round_layout round;            /* the solo round's: upload offsets relative to its place in the upload, download offsets
                                              relative to the download block, dev_off relative to round_off */
    int32_t n_models, reserved;
    size_t in_bytes;                       /* the solo call's upload */
    size_t out_bytes, solo_out_bytes;      /* host_out: the download, which reaches over the members' rows; the solo block in front */
    size_t flags_off, append_flags_off;    /* the edits' flag words in the download, as in the solo layouts (0: no such edit) */
    size_t member_off, member_stride;      /* host_out: member m's scores at member_off + m * member_stride */
    size_t arena_bytes, solo_arena_bytes, round_off, out_base;
    size_t ws_off[GCNN_GROUP_MAX], table_off;      /* internal: the members' forward workspaces and the launch tables in the arena */
    size_t table_bytes;                    /* host_staging holds this much */
} gcnn_lp_round_ensemble_layout;
int gcnn_lp_round_ensemble_layout_for(const gcnn_lp_rounds_edit_member* round /* host; only the sizes are read */, int32_t mode,
                                      int32_t n_models, gcnn_lp_round_ensemble_layout* layout /* host */);
int gcnn_lp_round_ensemble(const gcnn_lp_rounds_edit_member* round /* host */, int32_t mode, int32_t n_models,
                           const float* const* params /* host [n_models] */, const void* host_in, void* host_out, void* arena,
                           size_t arena_bytes, void* host_staging, double p_max, double p_max_ub, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCNN_HIP_H */
