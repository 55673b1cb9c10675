/* emgraph_hip.h — C-ABI of libemgraph_hip.so: the MI355X (gfx950) replacement for
 * bi-graph/Emgraph's per-batch hot path.
 *
 * The reference (pure Python on TensorFlow) has no FFI of its own; the entry points below are
 * what a ctypes binding inside the reference would call INSTEAD of the TF op groups cited at
 * each declaration (file:line relative to the reference tree).  INTEGRATION.md shows that stub.
 *
 * Conventions
 *   - every function returns 0 on success, a negative EMG_E* code otherwise; the message for the
 *     calling thread's last failure is emg_last_error().  No C++ exception crosses the ABI.
 *   - all pointers are DEVICE pointers on the current HIP device unless marked "host"; the caller
 *     owns every buffer (in our host code they are PyTorch-ROCm tensors); the library allocates
 *     nothing persistent — scratch comes from caller-provided workspaces sized by *_workspace_bytes.
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous and ordered on it.
 *   - embedding tables are float32 row-major with a row stride `ld` (in floats, ld >= k_int).
 *     ComplEx/HolE rows are [re(0:k) | im(k:2k)], k_int = 2k (ComplEx.py:224,288-290).
 *   - triples are int32 [n,3] row-major (s,p,o)  (EmbeddingModel.py:503-505).
 *   - eta-major negatives: negative row j (0 <= j < eta*B) corrupts positive j mod B
 *     (protocol.py:598).
 *
 * Supported sizes (tests/test_large_tables.py runs the entries on 16 GiB tables and / or on 25 165 829 rows — all but
 * emg_sampler_bind and a plan's fused riders, whose limits below come from reading the code)
 *   - every row stride (ld, ldc, ldq, ld_dst) and every row offset is int64_t: the BYTES of a table, an optimizer state table, a
 *     contribution buffer or a half-precision image are bounded by device memory only.
 *   - entity / relation ids, destination ids and candidate ids are int32_t >= 0, so a table indexed by them has fewer than 2^31
 *     rows; a corruption code keeps its id in the low 31 bits.  Entries that take a row count check it: "too many rows",
 *     "ids must fit 31 bits", "entity ids must fit int32" (emg_eval_topn: ent_offset + n_cand <= INT32_MAX),
 *     "too many entities" (emg_eval_rescore_pairs_tiles: slab rows < 2^32).
 *   - a grouping (emg_prepare_batch, emg_group_dest, emg_apply_*, emg_train_step) takes fewer than 2^31 contributions; it runs the
 *     counting backend while n_rows <= 16 n_contrib + 2^20 and rocPRIM's radix sort beyond, and emg_prepare_batch's bucket form
 *     serves tables of 262 144 .. 8 388 608 rows (4096 buckets of 2048 rows) — one row more and the counting form runs.
 *   - the prefilters pack an undecided pair as (row << 32) | entity: query rows and ent_offset + n_cand below 2^31.
 *   - passes over whole tables (emg_lp_*, emg_clip_rows, emg_init_table, emg_to_bf16 / _f16, emg_rows_normalize, the deferred
 *     passes) take int64_t rows; their grids stay below 2^32 blocks for any table that fits device memory.
 *   A size an entry cannot serve is refused with EMG_EINVAL and a message; nothing wraps silently.
 */
#ifndef EMGRAPH_HIP_H
#define EMGRAPH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMG_ABI_VERSION 9

#define EMG_OK 0
#define EMG_EINVAL (-1)   /* bad argument */
#define EMG_EHIP (-2)     /* HIP runtime error (message has hipGetErrorString) */
#define EMG_ENOSUP (-3)   /* combination not supported */

/* model ids: TransE.py:208-216 (norm 1 / 2), DistMult.py:201, ComplEx.py:288-298, HolE.py:189 */
#define EMG_TRANSE_L1 0
#define EMG_TRANSE_L2 1
#define EMG_DISTMULT 2
#define EMG_COMPLEX 3
#define EMG_HOLE 4
/* TransE with ANY positive order of the norm (TransE.py:208-216 hands `norm` to tf.norm as ord): f = -(sum |e_s + r_p - e_o|^ord)^(1/ord),
 * ord = +inf: the largest |component|; the `scale` argument of every call carries ord.  Inference: emg_score_triples and the
 * emg_eval_* / emg_rank_1vsall family at precision 0.  Training (round 4): the unfused step — emg_train_forward (eta > 0), emg_loss,
 * emg_train_backward_ex(fused_loss = -1: gradient -g sgn(d)|d|^(ord-1) / ||d||^(ord-1); ord = inf: shared by the tied maxima) — with
 * every gradient row through emg_apply_grouped (no in-place updates, no fused loss, no column slabs).  Generic kernels: orders 1
 * and 2 are EMG_TRANSE_L1 / _L2, the tuned (fused, MFMA- and v_sad-accelerated) models. */
#define EMG_TRANSE_P 5
/* RotatE (Sun et al., ICLR 2019; not in the reference: DESIGN.md 0, A-22): f = -sum_{j<k} |s_j r_j - o_j|, r_j = cos(theta_j) + i sin(theta_j)
 * — the paper's L1-of-moduli score without the constant gamma (the losses' `margin`; it moves no rank).  k_int = 2k (odd: EMG_EINVAL).
 * Entity rows are [re(k) | im(k)] as for ComplEx; a relation row has the same width: columns [0, k) hold the phases theta, columns
 * [k, 2k) are unused — zero after initialisation, and every kernel writes a zero gradient for them.  cos / sin are full-precision
 * sincosf (training moves the phases out of [-pi, pi]).  `scale` is unused: pass 1.0.
 *   query rows (emg_eval_build_queries)  object side q = s o r, subject side q = o o conj(r) (|s o r - e| = |s - e o conj(r)|, |r| = 1): the
 *              ComplEx formulas with p_r = cos(theta), p_i = sin(theta); sincosf once per (row, coordinate)
 *   canonical chain (1-vs-all: count, dense, top-N, filter, pos_int)  j ascending from acc = +0:  dr = q_re[j] - e_re[j], di = q_im[j] -
 *              e_im[j], m = sqrtf(fadd(fmul(dr, dr), fmul(di, di))), acc = fadd(acc, m); the score is -acc.  Unfused on purpose: every
 *              step is one correctly rounded IEEE operation
 *   gradient   w = s o r, d = w - o, m = |d|, u = d / m (u = 0 where m = 0):  df/ds = -u conj(r) = (-(u_re c + u_im sn), -(u_im c -
 *              u_re sn)),  df/do = +u,  df/dtheta = u_re w_im - u_im w_re,  relation columns [k, 2k): 0
 * Inference: emg_score_triples and the emg_eval_* / emg_rank_1vsall family at precision 0 (tiled exact kernels); the same counters,
 * bit for bit, from emg_eval_prefilter_rotate followed by emg_eval_rescore_pairs (the half-precision prefilter, below).  Training: the unfused
 * step of EMG_TRANSE_P — emg_train_forward, emg_loss, emg_train_backward_ex(fused_loss = -1), every gradient row through
 * emg_apply_grouped (no in-place updates, no fused loss, no factored contributions, no step records, no column slabs).
 * emg_eval_grid_count and emg_calib_step do not know this model. */
#define EMG_ROTATE 6
/* SimplE (Kazemi & Poole, NeurIPS 2018; not in the reference: DESIGN.md 0, A-27, 4.6), the averaged form.  k_int = 2k (odd: EMG_EINVAL).
 * An entity row is [h(k) | t(k)]: the entity's head role and tail role; a relation row is [r(k) | r_inv(k)].  With swap(x) exchanging the
 * two halves of a 2k-wide row,
 *   f(s, p, o) = 1/2 (sum_j h_s[j] r[j] t_o[j] + sum_j h_o[j] r_inv[j] t_s[j]) = scale * sum_{c < 2k} e_s[c] rel_p[c] swap(e_o)[c]
 * `scale` carries the 1/2 (pass 0.5; any finite value is taken as it is).
 *   query rows (emg_eval_build_queries, one fmul per column)  object side (s kept, scored against e_o): q = swap(rel_p) o swap(e_s);
 *              subject side (o kept, scored against e_s): q = rel_p o swap(e_o)
 *   canonical chain (1-vs-all: count, dense, top-N, filter, grid, grouped, lists, pos_int)  acc = fmaf(q[c], e[c], acc), c = 0 .. 2k - 1
 *              ascending from +0, then fmul(acc, scale): bit for bit what EMG_HOLE computes on the same q, e and scale.  Every entry
 *              point that consumes a prebuilt Q maps this id to that chain on entry (csrc/emg_common.hpp: chain_model) — emg_eval_count,
 *              emg_eval_filter_count, emg_eval_scores_dense, emg_eval_rescore_pairs (every form), the f16 prefilter and bf16 families,
 *              emg_eval_topn, emg_eval_grid_count, emg_eval_count_grouped, emg_eval_count_lists, emg_rank_1vsall (every precision mode)
 *   relation side (emg_eval_rel_count / _scores_dense)  the object-side chain with q built per (pair, relation, column) in registers
 *   gradient   (each times scale and the upstream dL/df)  df/de_s = rel o swap(e_o),  df/de_o = swap(rel o e_s),  df/drel = e_s o swap(e_o);
 *              a triple with s == o sends both entity contributions to the same row
 * Inference also through emg_score_triples.  Training: the unfused step of EMG_TRANSE_P (csrc/emg_simple.hip) — emg_train_forward,
 * emg_loss, emg_train_backward_ex(fused_loss = -1), every gradient row through emg_apply_grouped (no in-place updates, no fused loss,
 * no factored contributions, no step records, no column slabs); emg_train_step takes that route.  emg_calib_step and emg_shared_*
 * do not know this model.
 * Id 7 is unassigned ON PURPOSE: it is the id that names no model, and every entry point refuses it as unknown. */
#define EMG_SIMPLE 8

/* corruption side: protocol.py:598-608 ('s,o' is an alias of 's+o' there, :591-593) */
#define EMG_SIDE_S 0
#define EMG_SIDE_O 1
#define EMG_SIDE_SO 2

/* losses: losses/pairwise.py:66-70, nll.py:55-59, absolute_margin.py:66-70,
 * self_adversarial.py:90-112, nll_multiclass.py:70-81 */
#define EMG_LOSS_PAIRWISE 0
#define EMG_LOSS_NLL 1
#define EMG_LOSS_ABSOLUTE_MARGIN 2
#define EMG_LOSS_SELF_ADVERSARIAL 3
#define EMG_LOSS_MULTICLASS_NLL 4

/* score link (embedding_model_params['non_linearity'], EmbeddingModel.py:679-690 for the positives, :801-810 for the negatives,
 * :2135-2145 in predict): phi is applied to every score before the loss.  Gradients in the forms TF takes them:
 *   LINEAR    phi(x) = x                        phi' = 1
 *   TANH      y = tanh(x)                       phi' = 1 - y^2
 *   SIGMOID   y = 1 / (1 + e^-x)                phi' = y (1 - y)
 *   SOFTPLUS  y = log(1 + 9999 e^x)             phi' = 1 - 1 / (1 + 9999 e^x)   (the reference's custom_softplus, :90-96 — not the
 *             usual softplus; 9999 e^x overflows float32 from x = 79.6 on: y = inf, phi' = 1, as there) */
#define EMG_LINK_LINEAR 0
#define EMG_LINK_TANH 1
#define EMG_LINK_SIGMOID 2
#define EMG_LINK_SOFTPLUS 3

/* optimizers: training/sgd.py:97, momentum.py:63, adagrad.py:42, adam.py:45 (Keras rules) */
#define EMG_OPT_SGD 0
#define EMG_OPT_MOMENTUM 1
#define EMG_OPT_ADAGRAD 2
#define EMG_OPT_ADAM 3        /* Keras sparse apply == dense-equivalent: every row decays/updates */
#define EMG_OPT_ADAM_LAZY 4   /* touched rows only (not reference semantics; opt-in) */

/* score flags */
#define EMG_SCORE_FINAL 0     /* the model's score */
#define EMG_SCORE_PARTIAL 1   /* k-slice partial: TransE-L2 returns sum(d^2) (no -sqrt), HolE unscaled;
                                 finish with emg_finalize_scores after summing slices */

int emg_version(void);
const char* emg_last_error(void);
/* name of the compiled GPU target ("gfx950") */
const char* emg_target(void);
/* hash of the kernel sources the library was built from (the rocprofv3 evidence under profiles/ names the binary it measured) */
const char* emg_source_hash(void);
/* launches of the fused in-place SGD kernel's cache-policy form since the library was loaded (EMG_CACHE_POLICY) */
int64_t emg_cache_policy_launches(void);

/* ---- K1+K2: fused embedding gather + score (replaces EmbeddingModel._lookup_embeddings
 * :490-533 followed by Model._fn; the predict() path :2132-2133). out[n] f32. */
int emg_score_triples(int model, const float* ent, int64_t n_ent, int64_t ld_ent,
                      const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale,
                      const int32_t* spo, int64_t n, int32_t flags, float* out, void* stream);

/* finish partial scores in place (TransE-L2: -sqrt(x); HolE: scale*x; others unchanged) */
int emg_finalize_scores(int model, float scale, float* scores, int64_t n, void* stream);

/* ---- K3/K14: corruption draws (replaces the tf.random.uniform + mask logic of
 * generate_corruptions_for_fit, protocol.py:598-641).
 * codes[j] = replacement_entity | (keep_subject << 31), j in [0, B*eta).
 *   side S: keep_subject=0 (subject replaced); O: keep_subject=1; SO: Bernoulli(1/2) per row.
 *   replacement = idx if entities_list==NULL else entities_list[idx], idx ~ U{0..n_choices-1}
 *   drawn from Philox4x32-10(key=seed, counter=(j, draw_counter)); or, when inj_repl != NULL,
 *   idx = inj_repl[j] (and keep_subject = inj_mask[j] for side SO) — the "injected draws" mode
 *   used to reproduce the reference's golden vectors. */
int emg_corrupt_codes(int64_t B, int32_t eta, int side, int64_t n_choices,
                      const int32_t* entities_list, uint64_t seed, uint64_t draw_counter,
                      const int32_t* inj_mask, const int32_t* inj_repl, int32_t* codes, void* stream);

/* materialise the [B*eta,3] corruption array exactly as generate_corruptions_for_fit returns it
 * (protocol.py:643-656) from the positives and the codes */
int emg_corrupt_expand(const int32_t* pos, int64_t B, int32_t eta, const int32_t* codes,
                       int32_t* out_spo, void* stream);

/* ---- K1+K2+K4 for a training batch: scores of the B positives and of their eta*B negatives
 * given as codes; the [B*eta,3] array and the three gathered [n,k] temporaries of the reference
 * (EmbeddingModel.py:675-677,788-799) are never materialised.  Rows shared inside a positive
 * group (p and the kept side) are read once.  scores_neg is eta-major. */
int emg_train_forward(int model, const float* ent, int64_t n_ent, int64_t ld_ent,
                      const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale,
                      const int32_t* pos, int64_t B, int32_t eta, const int32_t* codes, int32_t flags,
                      float* scores_pos, float* scores_neg, void* stream);

/* ---- K5: loss value + dL/dscore (replaces Loss.apply, losses/loss.py:123-138, and TF autodiff
 * through it).  scores_neg is [n_sides*eta*B] (side-major, then eta-major); the positive is tiled
 * per side as EmbeddingModel.py:724-729,786-816.  *loss_accum (device f64) += loss.
 * g_pos[B] = sum over tiles/sides of dL/dpos, g_neg[n_sides*eta*B] = dL/dneg. */
int emg_loss(int loss, const float* scores_pos, const float* scores_neg, int64_t B, int32_t eta,
             int32_t n_sides, float margin, float alpha, double* loss_accum, float* g_pos, float* g_neg,
             void* stream);

/* ---- K7: adjoint of gather+score.  Writes per-group gradient rows (no atomics):
 *   contrib_ent[0*B+i] = dL/dE[s_i] from group i,  contrib_ent[1*B+i] = dL/dE[o_i],
 *   contrib_ent[2*B + j*B + i] = dL/dE[replacement of negative j of positive i]   (j < eta)
 *   contrib_rel[i] = dL/dR[p_i];   row stride ldc floats (>= k_int).
 * dest_ent[(2+eta)*B], dest_rel[B] receive the destination row ids of those rows. */
int emg_train_backward(int model, const float* ent, int64_t n_ent, int64_t ld_ent,
                       const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale,
                       const int32_t* pos, int64_t B, int32_t eta, const int32_t* codes,
                       const float* g_pos, const float* g_neg,
                       float* contrib_ent, float* contrib_rel, int64_t ldc,
                       int32_t* dest_ent, int32_t* dest_rel, void* stream);

/* destination ids of the (2+eta)*B entity / B relation contribution rows of a batch (layout above);
 * depends only on the batch ids and codes, so it can run ahead of the scoring kernels */
int emg_build_dest(const int32_t* pos, int64_t B, int32_t eta, const int32_t* codes,
                   int32_t* dest_ent, int32_t* dest_rel, void* stream);

/* Per-step values of a training step that a captured step graph cannot bake into kernel arguments: a DEVICE record
 * every kernel of the step reads instead (emg_prepare_args.ctl, emg_backward_args.ctl, emg_apply_args.ctl; NULL = the
 * values of the argument struct).  emg_plan_run fills an array of them per replay.  The batch is rows
 * [start, start + B) of the resident training set (the `pos` pointer of the call is then the set's row 0). */
typedef struct emg_step_ctl {
    int64_t start; int64_t B;
    uint64_t draw_counter0;                                  /* as emg_prepare_args.draw_counter0 */
    int64_t n_choices; const int32_t* entities_list;         /* corruption pool (n_choices 0: the call's) */
    int32_t step; int32_t reserved0;                         /* optimizer step number (>= 1) */
    float hyper_ent[8]; float hyper_rel[8];                  /* as emg_apply_rows' hyper; entries 0 (lr) and 5 (lr_t) are read */
} emg_step_ctl;

/* ---- everything about a training batch that does not depend on the tables, in one call (what the step
 * pipeline runs ahead on a side stream): the corruption codes of every corruption side (as emg_corrupt_codes,
 * side sd drawing with counter draw_counter0 + sd, codes side-major then eta-major), the destination ids of
 * all gradient rows (as emg_build_dest) and their stable grouping + singleton flags (as emg_group_dest) for
 * the entity and the relation table.  dest_ent / dest_rel start with n_extra_* caller-filled entries (the LP
 * regulariser's dense rows) followed by the batch's; the grouping covers both.
 * Batch-sharded multi-GPU training: `pos` holds rows [row_offset, row_offset + B) of a GLOBAL batch of B_global
 * positives; the draw of (negative jj, local row i) is then the one the whole batch would use for its row
 * jj * B_global + row_offset + i, so the negatives do not depend on how many GPUs share the batch.
 * B_global == 0 means B_global = B, row_offset = 0 (single GPU). */
typedef struct emg_prepare_args {
    const int32_t* pos; int64_t B; int32_t eta; int32_t n_sides; int32_t sides[4];
    int64_t n_choices; const int32_t* entities_list; uint64_t seed; uint64_t draw_counter0;
    const int32_t* inj_mask; const int32_t* inj_repl;       /* optional injected draws [n_sides*eta*B] */
    int32_t* codes;                                          /* out [n_sides*eta*B] */
    int32_t* dest_ent; int64_t n_extra_ent; int64_t n_ent;   /* out [n_extra_ent + (2+n_sides*eta)*B] */
    int32_t* dest_rel; int64_t n_extra_rel; int64_t n_rel;   /* out [n_extra_rel + B] */
    void* ws_ent; int64_t ws_ent_bytes; void* ws_rel; int64_t ws_rel_bytes;  /* emg_apply_workspace_bytes */
    uint8_t* single_flags;                                   /* optional out, per entity contribution row */
    int64_t B_global; int64_t row_offset;                    /* batch-sharded draws (see above); 0, 0 = whole batch */
    /* factored != 0 (bilinear models, n_extra_ent = 0): the entity workspace also receives, per sorted position, the
     * row of the 4*B-row contribution buffer its slot points at, and per negative slot its sorted position — what
     * emg_train_backward_ex (fac_ws_ent) and emg_apply_grouped_factored work from. */
    int32_t factored;
    /* ws_clean != 0: the caller zeroed the workspaces once (hipMemset of the whole buffer) and has used them only through
     * this library since — the grouping then skips re-zeroing its control region (every grouping leaves it zero) */
    int32_t ws_clean;
    /* layout_B > 0: the workspaces are laid out (and the launches sized) for layout_B >= B positives — a plan's capacity,
     * so that batches of different sizes share one layout; ctl: optional device record (see emg_step_ctl) */
    int64_t layout_B; const void* ctl;
} emg_prepare_args;
int emg_prepare_batch(const emg_prepare_args* args, void* stream);

/* ---- negative sampling: Bernoulli side choice and known-triple filtering.  NOT in the reference, whose
 * generate_corruptions_for_fit (protocol.py:598-641) tosses a fair coin for the side and draws the replacement uniformly
 * without looking at the graph; the precedents are OpenKE's `bern`, PyKEEN's BernoulliNegativeSampler / filtered=True and
 * LibKGE's `filtering`.  A sampler is BOUND to the library and read by every producer of corruption ids that has the
 * positives at hand: emg_prepare_batch (counting and bucket form), emg_corrupt_codes_sampled, and a plan (emg_plan_create
 * copies the binding of that moment: it is constant for the plan's run, and such a plan steps through emg_plan_step —
 * emg_plan_graph_ok answers 0).  emg_corrupt_codes has no positives and stays as it is; injected draws (inj_repl) bypass the
 * sampler as they bypass the draw.  With nothing bound every entry point computes what it always did, bit for bit.
 * These symbols are additions: EMG_ABI_VERSION stays 9, no existing structure or entry point changes.
 *
 * Corruption row j (the global draw index of emg_corrupt_codes / emg_prepare_batch, B_global / row_offset remap and per-side
 * restart included) of a positive (s, p, o), side call sd, counter c = draw_counter0 + sd, attempt t = 0 .. retries:
 *   o_t   = Philox4x32-10(c0 = (uint32) j, c1 = (uint32)(j >> 32) | t << 24, c2 = (uint32) c, c3 = (uint32)(c >> 32), key = seed)
 *   idx_t = mulhi64(o_t[2] << 32 | o_t[1], n_choices)                (attempt 0 is emg_corrupt_codes' draw; j < 2^56)
 *   side  (EMG_SIDE_SO only; S / O stay forced)  keep_subject = o_0[0] & 1 (keep_thr == NULL), else o_0[3] < keep_thr[p] with
 *         keep_thr[p] = min(2^32 - 1, floor(|S_p| 2^32 / (|S_p| + |O_p|))), S_p / O_p the distinct subjects / objects of relation p:
 *         TransH's P(replace the subject) = tph / (tph + hpt) (Wang et al. 2014).  Decided once, from attempt 0.
 *   filter (n_known > 0)  the candidate of attempt t is (pool[idx_t], p, o) or (s, p, pool[idx_t]), pool = entities_list or the
 *         identity; the first t whose candidate's key (s n_rel + p) n_ent + o is not among known_keys is taken, the last one
 *         (t = retries) if all are known.  A row whose attempt-0 candidate is unknown gets exactly the unfiltered negative.
 *   stats (optional)  += {rows drawn, rows whose final attempt is > 0, rows whose final candidate is known}.
 * Device arrays: keep_thr uint32 [n_rel] or NULL; known_keys uint64 [n_known], ascending and distinct, or NULL with
 * n_known = 0; stats uint64 [3], 8-byte aligned, or NULL.  They stay the caller's and must outlive every call (and plan)
 * that reads the binding.  `size` = sizeof(emg_sampler) comes first: the structure may grow at its end (it has: pool_ptr / pool_idx
 * below; the size of the first layout is still accepted).
 * emg_sampler_bind(NULL) unbinds.  EMG_EINVAL: bad sizes, retries outside 1..255 with a filter; EMG_ENOSUP:
 * n_ent^2 n_rel >= 2^63 with a filter (the key would not fit).  The binding is one per process and NOT re-entrant: a second bind replaces
 * the first, and bind ... unbind sequences of two threads must not interleave (ask emg_sampler_bound first). */
typedef struct emg_sampler {
    int64_t size;
    const uint32_t* keep_thr;
    const uint64_t* known_keys; int64_t n_known;
    int64_t n_ent; int64_t n_rel;
    int32_t retries; int32_t reserved0;
    uint64_t* stats;
    /* ---- grown at the end (a caller passing the size up to here gets exactly the behaviour above) ----
     * TYPED negatives (PyKEEN's pseudo-typed negative sampler; Krompass et al. 2015): the replacement of a corruption of relation
     * p is drawn from the entities observed on that side of p.  One CSR over 2 n_rel groups, group g = 2 p + keep_subject
     * (g = 2 p: the DOMAIN pool, the subject is replaced; g = 2 p + 1: the RANGE pool, the object is replaced): pool_ptr int64
     * [2 n_rel + 1] ascending from 0, pool_idx int32 global entity ids (device arrays, the caller's, as the others).  With
     * len = pool_ptr[g + 1] - pool_ptr[g] > 0, attempt t draws idx_t = mulhi64(o_t[2] << 32 | o_t[1], len) and takes
     * pool_idx[pool_ptr[g] + idx_t] — the same Philox words, another multiplier and lookup; len == 0, or p outside [0, n_rel),
     * draws as above (n_choices / entities_list).  The side is decided first, as above; redraws come from the same pool; a pool of
     * one member may return the positive's own entity (taken as it is; counted as known_left under a filter).
     * pool_ptr == NULL: no pools, today's draws bit for bit.  With pools `stats` is uint64 [4]: [3] += rows drawn from a non-empty
     * pool.  Pools together with entities_list are refused on the host side (emgraph_amd), not here. */
    const int64_t* pool_ptr; const int32_t* pool_idx;
} emg_sampler;
int emg_sampler_bind(const emg_sampler* s);
int emg_sampler_bound(void);   /* 1: a sampler is bound */
/* emg_corrupt_codes for the corruptions of the B positives `pos` (int32 [B, 3]; row j corrupts positive j mod B,
 * protocol.py:598) through the bound sampler; with nothing bound: emg_corrupt_codes itself. */
int emg_corrupt_codes_sampled(const int32_t* pos, int64_t B, int32_t eta, int side, int64_t n_choices,
                              const int32_t* entities_list, uint64_t seed, uint64_t draw_counter,
                              const int32_t* inj_mask, const int32_t* inj_repl, int32_t* codes, void* stream);

/* ---- K5+K7 fused / extended backward.  One pass over the (3+eta) rows of each positive group:
 *   fused_loss >= 0 (EMG_LOSS_PAIRWISE | EMG_LOSS_NLL | EMG_LOSS_ABSOLUTE_MARGIN — the losses whose
 *       dL/dneg_j depends only on (pos_i, neg_j)): scores, loss (accumulated into *loss_accum) and
 *       dL/dscore are computed in the kernel; scores_*_out optional.
 *   fused_loss < 0: dL/dscore is read from g_pos / g_neg (any loss; see emg_loss).
 *   single_ent != NULL: uint8 per entity contribution slot (from emg_group_dest); slots flagged 1 have a
 *       destination hit exactly once in this batch and are applied to the table IN PLACE (optimizer `opt`,
 *       hyper = 8 floats as emg_apply_rows) instead of being written to contrib_ent — finish with
 *       emg_apply_grouped(..., skip_single=1).
 *   bw_scores_* : optional global final scores, used only by TransE-L2 when `ent`/`rel` are column
 *       slices (k-sharded multi-GPU) so that the norm is the full one.
 * Relation gradients always go to contrib_rel. */
typedef struct emg_backward_args {
    int32_t model; int32_t k_int; float scale; int32_t eta;
    const float* ent; int64_t n_ent; int64_t ld_ent;
    const float* rel; int64_t n_rel; int64_t ld_rel;
    const int32_t* pos; int64_t B; const int32_t* codes;
    int32_t fused_loss; float margin; double* loss_accum;
    const float* g_pos; const float* g_neg;
    const float* bw_scores_pos; const float* bw_scores_neg;
    float* scores_pos_out; float* scores_neg_out;
    float* contrib_ent; float* contrib_rel; int64_t ldc;
    const uint8_t* single_ent; int32_t opt; int32_t step; float hyper[8];
    float* ent_state0; float* ent_state1; int32_t* tag_ent;
    /* FACTORED entity contributions (NULL = off; DistMult / ComplEx / HolE only).  The gradient row of a negative's
     * replacement entity is  gi * q, q being one of the TWO query rows of its triple group (object side: q(s, p);
     * subject side: q(p, o)) — so instead of eta full rows per group the kernel writes q once per side and ONE float
     * per negative.  fac_ws_ent = the entity workspace of the emg_prepare_batch call (factored = 1) for this batch: the
     * float goes straight to the sorted position of the negative's slot there (slots updated in place write nothing).
     * contrib_ent then has 4*B rows: [0,B) subject rows, [B,2B) object rows, [2B,3B) q object side, [3B,4B) q subject
     * side, and the table apply is emg_apply_grouped_factored (same sums, same order, same bits: it adds the rounded
     * product gi * q exactly where the unfactored path adds the stored row). */
    void* fac_ws_ent; int64_t fac_ws_ent_bytes;
    int64_t layout_B; const void* ctl;   /* as in emg_prepare_args: layout of fac_ws_ent; device record, pos = row 0 of the resident set */
    double* lp_accum;   /* folded LP with in-place updates (below): += sum |w|^p (pre-update) over the rows updated in place */
    /* lr_hist != NULL (EMG_OPT_ADAM in place with inplace_window, fused loss, deferred dense pass — see emg_deferred_catchup): the rows of SINGLETON
     * NEGATIVES are as of tag_ent[row]; the kernel fetches (w, m, v) of such a row together, replays the steps tag + 1 .. step - 1 in
     * registers (the dense pass's update with g = 0 and lr_hist[s]), scores the row, applies this step's update and writes
     * (w, m, v, tag = step): one read and one write of the three rows where catch-up + scoring + apply moved twelve.  The same for
     * singleton subject / object rows (replayed before the group's queries are built).  Finish with emg_apply_grouped_ex(skip_single
     * = 1) after emg_deferred_catchup(..., skip_single_from = 0) brought every other row of the batch up to date. */
    const float* lr_hist;
    /* inplace_window != 0 (stateful optimizers; fused loss; 16-byte rows of at most 64 chunks, per half for complex models): a
     * singleton negative's optimizer state rows are fetched together with its table row in the kernel's rolling window — the update
     * waits for nothing (0: the state is read chunk by chunk at the update).  The subject / object singletons are updated in place too
     * (without lr_hist: at the group's end, state read chunk by chunk; with lr_hist: replayed at the group's start, parked in LDS,
     * updated at its end): finish with skip_single = 1.  Required by lr_hist. */
    int32_t inplace_window;
    /* loss_slots: 0 / 1: loss_accum is ONE double.  A power of two n > 1: loss_accum points to n doubles, workgroup b of the fused
     * kernel adds its partial sum to loss_accum[b & (n - 1)], the batch's loss is their sum.  (One double atomic per workgroup to
     * ONE address retires one per ~10 ns at the memory side of the eight L2s: the 680 workgroups of a 20 us launch — the reference's
     * own configurations — all arrive within its last microseconds; measured 5 of C2's 22 us.) */
    int32_t loss_slots;
    /* ABI 9 — score link and FocusE edge weights (EmbeddingModel.py:679-722, 801-816), fused loss only (any other loss: emg_link_scores /
     * emg_link_grads around emg_loss).  link: EMG_LINK_*.  edge_w != NULL: float [B], indexed like `pos` (with a device record: the
     * resident set's row 0, advanced by ctl->start): w_i in [0, 1], the row's numeric edge value after normalisation, mean over its
     * columns.  sw: the structure weight of this step (:694-714).  The positive's score enters the loss as
     * (sw + (1 - sw)(1 - w_i)) phi(pos_i), each of its negatives' as (sw + (1 - sw) w_i) phi(neg) (:716-722, 812-813), and dL/dscore
     * is scaled by weight * phi' on its way back.  link = EMG_LINK_LINEAR and edge_w = NULL: none of it runs (today's bits).
     * scores_pos_out / scores_neg_out receive the raw scores either way. */
    int32_t link; float sw; const float* edge_w;
} emg_backward_args;
/* hyper[6] = lambda, hyper[7] = p of an LP regulariser folded into the update (see emg_apply_grouped): with single_ent != NULL
 * only for opt = EMG_OPT_SGD — a singleton row is then updated in place with g + lambda p |w|^(p-1) sign(w), the rule the
 * apply uses for every other row, tagged, and its |w|^p added to *lp_accum; with a stateful optimizer and a regulariser
 * pass single_ent = NULL (every row through emg_apply_grouped). */
int emg_train_backward_ex(const emg_backward_args* args, void* stream);
/* The dry run of emg_train_backward_ex: every check and the whole decision of which kernel would run for `args` (have_riders != 0:
 * as a step of a plan that has preparation stages of later batches to place), with the return code and emg_last_error() text of the
 * real call — and no launch.  No device is touched and none of the pointers in `args` is followed (they are compared with NULL and
 * tested for alignment only), so the decision is testable on a host without a GPU (tests/test_step_forms.py).  out[0] pass (1
 * backward from external dL/dscore, 2 fused), [1] model, [2] floats per chunk (4: 16-byte rows, 1: scalar rows), [3] chunks per
 * lane (0 with blocks 0: nothing to launch), [4] lanes per group, [5] in-place form (0 none, 1 SGD, 2 stateful, 3 SGD + LP, 4 / 5
 * window with one / two state rows, 6 window with lagging Adam rows, 7 SGD + LP with lagging rows), [6] flags: 1 cache-policy form,
 * 2 score link / edge weights, 4 riders carried, 8 riders launched alone first, [7] launches: column blocks of 512 (1 unless
 * wide-row backward: [3], [4] are the full blocks' shape, the last, narrower block takes its own).  All zero on failure. */
int emg_train_backward_form(const emg_backward_args* args, int32_t have_riders, int32_t out[8]);

/* ---- score link and FocusE edge weights for the step that is NOT fused (emg_train_forward -> emg_loss -> emg_train_backward_ex with
 * fused_loss = -1; EmbeddingModel.py:679-722, 801-816; link / edge_w / sw as in emg_backward_args).
 * emg_link_scores: the raw scores of a batch — scores_pos [B], scores_neg [eta_total * B], side-major then eta-major, the layout of
 *   emg_loss — become the effective scores weight * phi(score) IN PLACE, and fac_pos [B] / fac_neg [eta_total * B] receive
 *   weight * phi'(score) (edge_w = NULL: weight 1);
 * emg_link_grads: g_pos / g_neg (emg_loss's dL/d effective score) *= fac_pos / fac_neg: dL/d raw score, what the backward call takes. */
int emg_link_scores(int32_t link, const float* edge_w, float sw, float* scores_pos, float* scores_neg, int64_t B,
                    int32_t eta_total, float* fac_pos, float* fac_neg, void* stream);
int emg_link_grads(float* g_pos, float* g_neg, const float* fac_pos, const float* fac_neg, int64_t B, int32_t eta_total,
                   void* stream);

/* ---- K8 in two halves (emg_apply_rows = both):
 * emg_group_dest: stable grouping of (dest, index) into `workspace` (+ optional singleton flags[n]) — a counting sort over
 *   the table rows (histogram, one scan, scatter, in-segment ordering: csrc/emg_group.hip) that also emits the segment
 *   descriptors emg_apply_grouped works from; keys wider than 16 n + 2^20 go through a device radix sort instead;
 * emg_apply_grouped: segmented sum + optimizer update using that workspace; skip_single != 0 skips
 * length-1 segments (already applied in place by emg_train_backward_ex). */
int emg_group_dest(const int32_t* dest, int64_t n, int64_t n_rows, void* workspace, int64_t workspace_bytes,
                   uint8_t* single_flags, void* stream);
/* emg_group_dest with an explicit order: a destination's contributions are summed in ascending order_key (distinct within a
 * destination) instead of ascending index — the batch-sharded multi-GPU step: the owner of a table range receives gradient rows
 * from every rank and adds them in the order of their slots in the GLOBAL batch.  Counting backend only (EMG_ENOSUP otherwise).
 * Apply with emg_apply_grouped_factored(contrib = the received rows): it reads row i through the workspace's source array. */
int emg_group_dest_keyed(const int32_t* dest, const uint32_t* order_key, int64_t n, int64_t n_rows, void* workspace,
                         int64_t workspace_bytes, void* stream);
int emg_apply_grouped(int opt, float* table, int64_t n_rows, int64_t ld, int32_t k_int,
                      float* state0, float* state1, int32_t* tag, int32_t step,
                      const float* contrib, int64_t ldc, int64_t n_contrib, int32_t skip_single,
                      const float* hyper, double* lp_accum, void* workspace, int64_t workspace_bytes, void* stream);
/* emg_apply_grouped for an entity table whose contributions the backward kernel wrote FACTORED (emg_backward_args.
 * fac_ws_ent = this workspace, grouped by emg_prepare_batch with factored = 1): n_contrib = (2 + eta) * B contribution
 * slots, `contrib` the 4*B-row buffer. */
int emg_apply_grouped_factored(int opt, float* table, int64_t n_rows, int64_t ld, int32_t k_int,
                               float* state0, float* state1, int32_t* tag, int32_t step,
                               const float* contrib, int64_t ldc, int64_t n_contrib, int32_t skip_single,
                               const float* hyper, double* lp_accum, void* workspace, int64_t workspace_bytes, void* stream);
/* emg_apply_grouped[_factored] with every argument in a struct, and the PAIR form: two tables (a training step's entity
 * and relation table) through shared launches — one window kernel over both groupings, one task kernel over both task
 * lists.  Same results as two calls; where the two shapes cannot share a launch (scalar or <= 16-chunk rows, only one of
 * the workspaces sized for tasks) it IS two calls. */
typedef struct emg_apply_args {
    int32_t opt; int32_t k_int; float* table; int64_t n_rows; int64_t ld;
    float* state0; float* state1; int32_t* tag; int32_t step; int32_t skip_single;
    const float* contrib; int64_t ldc; int64_t n_contrib;
    float hyper[8]; double* lp_accum; void* workspace; int64_t workspace_bytes;
    int32_t factored;
    int32_t table_index;                 /* 0 entity / 1 relation table: which hyper-parameters of `ctl` apply */
    int64_t layout_n; const void* ctl;   /* layout_n > 0: contribution slots the workspace was laid out for (>= n_contrib); device record */
    int32_t deferred_dense; int32_t reserved1;   /* 1: no dense pass (Keras Adam's decay, the LP regulariser's): the caller runs emg_deferred_catchup, below;
                                                  * 2: the same, and the catch-up ran with w_only (m, v of the destinations lag behind w) */
} emg_apply_args;
int emg_apply_grouped_ex(const emg_apply_args* args, void* stream);
int emg_apply_grouped_pair(const emg_apply_args* a, const emg_apply_args* b, void* stream);
/* DEFERRED dense pass.  Keras Adam (training/adam.py:31-48) decays m, v and moves w of EVERY row every step; a folded LP
 * regulariser (regularizers/lp.py:107-113) gives every row a gradient every step: on a 1M x 400 table that is 3.2 - 9.6 GB
 * read + written per step.  Deferred: a row nothing touches keeps (w, state) as of tag[row], the last step it was written
 * at; before a batch is scored, emg_deferred_catchup replays the missed steps tag[row]+1 .. upto — the dense pass's own
 * update (g = the regulariser's gradient alone) with THAT step's learning rate lr_hist[step] (lr_t for Adam, lr otherwise),
 * the same float operations in the same order, so the same bits — for exactly the rows the batch will read and update: the
 * destinations of the grouping in `workspace` (emg_prepare_batch's, counting backend).  The apply then runs with
 * deferred_dense = 1 (no dense pass).  emg_deferred_materialize does the same for every row (before the tables are read,
 * and — with a regulariser — before a loss is reported: *lp_accum += sum |w|^p of every replayed step).  hyper: the 8 values
 * of emg_apply_grouped (hyper[0] / hyper[5] are replaced per step by lr_hist).
 * w_only = 1 (EMG_OPT_ADAM, no regulariser; the apply must then run with deferred_dense = 2): for the destinations the apply
 * finishes with one wave each (the grouping's multi / single lists, gaps of at most 64 steps) only w is written back — m, v
 * and tag[row] stay as of the row's last write, and the apply redoes their decay over the missed steps in registers
 * (two multiplications per element and step) instead of this call writing and the apply re-reading both state rows.
 * Same bits.
 * skip_single_from >= 0: singleton destinations whose contribution slot is >= it are left alone — the scoring kernel replays them
 * itself as it gathers them (emg_backward_args.lr_hist: 0 = every singleton); < 0: none are. */
int emg_deferred_catchup(int opt, float* table, int64_t n_rows, int64_t ld, int32_t k_int, float* state0, float* state1,
                         int32_t* tag, const float* hyper, const float* lr_hist, int32_t upto_step, double* lp_accum,
                         const void* workspace, int64_t workspace_bytes, int64_t layout_n, int32_t w_only, int64_t skip_single_from,
                         void* stream);
int emg_deferred_materialize(int opt, float* table, int64_t n_rows, int64_t ld, int32_t k_int, float* state0, float* state1,
                             int32_t* tag, const float* hyper, const float* lr_hist, int32_t upto_step, double* lp_accum,
                             void* stream);
/* LP regulariser folded into the optimizer step (hyper[6] = lambda != 0, hyper[7] = p): the penalty covers the FULL
 * table (regularizers/lp.py:107-113, EmbeddingModel.py:818-820), so its gradient lambda*p*|w|^(p-1)*sign(w) reaches
 * every row.  Rows with contributions (and rows the backward kernel updates in place) add it to their summed
 * gradient; rows nothing touched in this step (tag[r] != step) are visited by ONE dense pass that applies the
 * optimizer with that gradient alone.  *lp_accum (device double, may be NULL) += sum of |w|^p over all rows at their
 * pre-update values — the caller multiplies by lambda for the loss.  Needs `tag`. */

/* ---- K8: deterministic row-sparse optimizer apply.  Sorts (dest, index) (stable radix sort),
 * sums each destination's contribution rows in index order and updates that table row once.
 * state0/state1: momentum buffer | adagrad accumulator | adam m, v  (same shape/stride as the table;
 * NULL when unused).  `tag` int32[n_rows] scratch owned by the caller (persistently, zero-initialised
 * once) marks rows touched in step `step` (>=1) — needed by EMG_OPT_ADAM's dense pass.
 * hyper: HOST pointer to 8 floats {lr, momentum, beta1, beta2, eps, lr_t, lp_lambda, lp_p} read at call time
 * (lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t), Adam only; lp_lambda = 0: no regulariser folded in, see emg_apply_grouped). */
int64_t emg_apply_workspace_bytes(int64_t n_contrib, int64_t n_rows);
/* the same plus scratch for the long-segment reduction (destinations hit by more than 64 contributions in a batch —
 * hub entities of a skewed graph, relation rows — are summed as 64-row blocks by a whole workgroup instead of by one
 * wave); with the smaller workspace above such segments are summed by a single wave (slow, same reduction order only
 * for segments of up to 64 rows) */
int64_t emg_apply_workspace_bytes_ex(int64_t n_contrib, int64_t n_rows, int32_t k_int);
int emg_apply_rows(int opt, float* table, int64_t n_rows, int64_t ld, int32_t k_int,
                   float* state0, float* state1, int32_t* tag, int32_t step,
                   const float* contrib, int64_t ldc, const int32_t* dest, int64_t n_contrib,
                   const float* hyper, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- K6: LP regulariser over FULL tables (regularizers/lp.py:107-113): *loss_accum +=
 * lambda * sum |W|^p, and (if grad_scale_lr != 0) the SGD-style in-place update
 * W -= grad_scale_lr * lambda * p * |W|^(p-1) * sign(W). */
int emg_lp_regularizer(float* table, int64_t n_rows, int64_t ld, int32_t k_int, float lambda, int32_t p,
                       float grad_scale_lr, double* loss_accum, void* stream);

/* K6, optimizer-agnostic form: the regulariser's gradient as n_rows extra contribution rows
 * (contrib[r] = lambda*p*|W[r]|^(p-1)*sign(W[r]), dest[r] = r) to be appended to the batch's
 * contributions before emg_apply_rows; also accumulates the loss term. */
int emg_lp_grad_rows(const float* table, int64_t n_rows, int64_t ld, int32_t k_int, float lambda, int32_t p,
                     float* contrib, int64_t ldc, int32_t* dest, double* loss_accum, void* stream);

/* ---- K9: optional row-norm clip after a batch (EmbeddingModel.py:1371-1380, clip_by_norm axes=1) */
int emg_clip_rows(float* table, int64_t n_rows, int64_t ld, int32_t k_int, float max_norm, void* stream);
/* rows[j] -> table[ids[j]] for 0 <= ids[j] < n_rows (distinct ids; others skipped): the multi-GPU batch-sharded step with the
 * optimizer state sharded by OWNER writes the owners' updated rows into every replica with it (no reference counterpart: the
 * reference has no distributed code; the update itself is training/{sgd,momentum,adagrad}.py) */
int emg_scatter_rows(float* table, int64_t n_rows, int64_t ld, int32_t k_int, const float* rows, int64_t ldr,
                     const int32_t* ids, int64_t n, void* stream);
/* initializers/{glorot_uniform,uniform,normal}.py on the device: kind 0 = U[a, b), 1 = N(mean a, std b); element (r, c)
 * takes word (c & 3) of Philox4x32-10(counter (r * k_int + c) / 4, stream_id, seed), so a table is a pure function of
 * (seed, stream_id, shape) — the same on any number of GPUs.  The reference draws from TensorFlow's generators (cannot
 * be reproduced: parity-unpinned); Glorot-uniform is U(+-sqrt(6 / (rows + cols))) (glorot_uniform.py:59-74). */
int emg_init_table(int kind, float* table, int64_t n_rows, int64_t ld, int32_t k_int, float a, float b,
                   uint64_t seed, uint64_t stream_id, void* stream);

/* ====================== filtered 1-vs-all ranking (K10-K13) ======================
 * side_mode: 0 's' | 1 'o' | 2 's+o' | 3 's,o'.  Query rows: for modes 2,3 rows [0,n_q) are the
 * OBJECT-side queries (s,p,?) and rows [n_q,2n_q) the SUBJECT-side queries (?,p,o) — the block
 * order of generate_corruptions_for_eval (protocol.py:511-518); modes 0/1 have n_q rows. */
#define EMG_EVAL_S 0
#define EMG_EVAL_O 1
#define EMG_EVAL_SPO 2
#define EMG_EVAL_S_O 3

/* Build the query matrix Q[n_rows, ldq] and the positive's comparison integer
 * pos_int[n_rows] = int32(score_pos * 1e5) (EmbeddingModel.py:1865-1866,2010-2014), with the
 * positive scored through the SAME arithmetic as its corruptions (see DESIGN.md "canonical order").
 * Query vectors: DistMult q=p*x; ComplEx/HolE the Re/Im-hoisted vectors (SURVEY B-2);
 * TransE object side q=s+p, subject side q=o-p. */
int emg_eval_build_queries(int model, const float* ent, int64_t n_ent, int64_t ld_ent,
                           const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale,
                           const int32_t* test_spo, int64_t n_q, int side_mode,
                           float* Q, int64_t ldq, int32_t* pos_int, void* stream);

/* Count, for every query row, the candidates whose comparison integer is > / == the positive's
 * (perform_comparision, EmbeddingModel.py:2010-2033; worst = gt+eq, best = gt,
 * middle = gt+ceil(eq/2) are formed by the caller).  Candidates are rows [0,n_cand) of `ent`
 * (an entity slab) or, if cand != NULL, rows cand[0..n_cand) of it.  cnt_gt/cnt_eq int32[n_rows]
 * are ACCUMULATED (zero them first; sum over slabs / GPUs).
 * precision: must be 0 = fp32 (exact f32-MFMA for DistMult/ComplEx/HolE; f32 VALU for TransE); any other value
 *            returns EMG_ENOSUP.  ent_bf16 / ld_bf16 are ignored (reserved): the bf16 MFMA throughput mode has its
 *            own entry points below (emg_eval_count_bf16 ...) because its operands are the bf16 copies. */
int emg_eval_count(int model, const float* Q, int64_t ldq, const int32_t* pos_int, int64_t n_rows,
                   const float* ent, int64_t n_cand, int64_t ld_ent, const int32_t* cand,
                   int32_t k_int, float scale, int precision, const void* ent_bf16, int64_t ld_bf16,
                   int32_t* cnt_gt, int32_t* cnt_eq, void* stream);

/* Same counts restricted to each query row's filter list (CSR: filt_ptr int64[n_rows+1],
 * filt_idx int32 GLOBAL entity ids; `ent` points at global row `ent_offset` and holds n_local rows;
 * entries outside [ent_offset, ent_offset+n_local) are skipped so every slab owner can be handed
 * the same global list) — replaces the tf.gather(scores, indices_obj/sub) + perform_comparision of
 * EmbeddingModel.py:1942-1963 and the SQLite lookups feeding it (sqlite_adapter.py:449-508).
 * fcnt_gt/fcnt_eq are ACCUMULATED. */
int emg_eval_filter_count(int model, const float* Q, int64_t ldq, const int32_t* pos_int, int64_t n_rows,
                          const float* ent, int64_t n_local, int64_t ld_ent, int64_t ent_offset,
                          int32_t k_int, float scale, int precision,
                          const int64_t* filt_ptr, const int32_t* filt_idx,
                          int32_t* fcnt_gt, int32_t* fcnt_eq, void* stream);

/* Debug/verification: dense scores S[n_rows, lds>=n_cand] through the SAME kernels as
 * emg_eval_count (small sizes only). */
int emg_eval_scores_dense(int model, const float* Q, int64_t ldq, int64_t n_rows,
                          const float* ent, int64_t n_cand, int64_t ld_ent, const int32_t* cand,
                          int32_t k_int, float scale, int precision, const void* ent_bf16, int64_t ld_bf16,
                          float* S, int64_t lds, void* stream);

/* ---- top-N completions: the 1-vs-all scoring of EmbeddingModel.py:1856-1866 with "keep the best top_n" in place of
 * "count against the positive" (csrc/emg_topn.hip).  For every query row the top_n best candidates outside the row's
 * exclusion list, in the TOTAL ORDER: higher score first; -0 == +0; a NaN score below every number, NaNs equal among
 * themselves; equal scores by ascending global entity id.  A score is the canonical chain with the model's final step,
 * bit-equal to the entry emg_eval_scores_dense(precision 0) writes for the same Q and table.
 *   candidates: rows [0, n_cand) of `ent` (global id ent_offset + j) or, if cand != NULL, rows cand[j] of it (global id
 *               cand[j]; distinct ids);
 *   excl_ptr int64[n_rows + 1] / excl_idx int32: CSR of global ids a row must not return, ASCENDING within a row;
 *               both may be NULL (nothing excluded);
 *   ent_chunk:  candidates per selection chunk, rounded up to a multiple of 256; 0 = the library's choice.  Every (row,
 *               chunk) leaves its top_n in `ws` (emg_eval_topn_ws_bytes of the same sizes; 8-byte aligned), a second
 *               launch merges them.  Both launches are asynchronous on `stream`;
 *   out_ids int32 / out_scores float [n_rows, top_n]: a row with fewer than top_n candidates is padded with (-1, -inf);
 *               n_cand == 0 gives padding only.
 * 1 <= top_n <= EMG_TOPN_MAX, EMG_EINVAL otherwise (also for a workspace that is too small). */
#define EMG_TOPN_MAX 128
/* Top-N workspace of EmbeddingModel.py:1856-1866's 1-vs-all scoring (see emg_eval_topn); negative EMG_E* on bad sizes. */
int64_t emg_eval_topn_ws_bytes(int64_t n_rows, int64_t n_cand, int32_t top_n, int64_t ent_chunk);
int emg_eval_topn(int model, const float* Q, int64_t ldq, int64_t n_rows,
                  const float* ent, int64_t n_cand, int64_t ld_ent, const int32_t* cand, int64_t ent_offset,
                  int32_t k_int, float scale, int32_t top_n,
                  const int64_t* excl_ptr, const int32_t* excl_idx,
                  int64_t ent_chunk, void* ws, int64_t ws_bytes, int32_t* out_ids, float* out_scores, void* stream);

/* ---- grid counts: the 1-vs-all scoring of EmbeddingModel.py:1856-1866 compared as EmbeddingModel.py:2010-2033 compares it,
 * but against MANY thresholds per query row instead of one positive (csrc/emg_grid.hip; discover_facts' grid ranking).
 * With I(r, e) = (int)(score(Q_r, ent_e) * 1e5f) — the score is the canonical chain with the model's final step, bit-equal to
 * the entry emg_eval_scores_dense(precision 0) writes for that pair; the product is one rounded f32 multiplication, as in
 * emg_eval_count — the call writes (not accumulates)
 *   cnt_gt[r, t] = #{e in [0, n_ent), e not in excl(r) : I(r, e) >  I(r, thr_ids[t])}
 *   cnt_eq[r, t] = #{e in [0, n_ent), e not in excl(r) : I(r, e) == I(r, thr_ids[t])}        int32 [n_rows, n_thr].
 * The threshold entity is counted like any other entity: one tie, unless it is excluded.
 *   Q [n_rows, ldq]: query rows as emg_eval_build_queries makes them;
 *   thr_ids int32[n_thr]: entity ids in [0, n_ent), shared by all rows, repeats allowed, 1 <= n_thr <= EMG_GRID_THR_MAX;
 *   excl_ptr int64[n_rows + 1] / excl_idx int32: CSR of global ids a row does not count, ASCENDING within a row; both may be
 *               NULL (nothing excluded) — the convention of emg_eval_topn;
 *   ws: emg_eval_grid_ws_bytes(n_rows, n_thr) bytes, 4-byte aligned: the rows' sorted distinct thresholds.
 * Two launches, asynchronous on `stream`; no host read, no allocation.  EMG_EINVAL: unknown model, n_thr outside
 * [1, EMG_GRID_THR_MAX], n_ent < 1, bad strides, a workspace that is too small.  Additions: EMG_ABI_VERSION stays 9. */
#define EMG_GRID_THR_MAX 256
/* Workspace of the many-threshold form of EmbeddingModel.py:1856-1866 / :2010-2033 (see emg_eval_grid_count):
 * n_rows * (2 n_thr + 1) * 4 bytes; negative EMG_E* on bad sizes. */
int64_t emg_eval_grid_ws_bytes(int64_t n_rows, int32_t n_thr);
int emg_eval_grid_count(int model, const float* Q, int64_t ldq, int64_t n_rows,
                        const float* ent, int64_t n_ent, int64_t ld_ent, int32_t k_int, float scale,
                        const int32_t* thr_ids, int32_t n_thr,
                        const int64_t* excl_ptr, const int32_t* excl_idx,
                        void* ws, int64_t ws_bytes, int32_t* cnt_gt, int32_t* cnt_eq, void* stream);

/* ---- relation prediction: the 1-vs-all scoring of EmbeddingModel.py:1856-1866 turned to the third side of a triple — every
 * candidate RELATION scored against a (subject, object) pair (csrc/emg_relrank.hip; not in the reference).
 * ONE TRIPLE, ONE SCORE: the score of (s, r, o) is the canonical chain of the object-side query row emg_eval_build_queries
 * writes for (s, r) against row o of `ent`, with the model's final step: bit-equal to the entry emg_eval_scores_dense(precision
 * 0) holds for that query row and entity, so a triple compares identically whichever side is ranked.  All seven model ids.
 *   test int32 [n_rows, 3]: (s, p, o) per row; the kernels read s and o only;
 *   candidates: rows [0, n_cand) of `rel` (n_cand <= n_rel) or, if cand_rel != NULL, rows cand_rel[j] of it (distinct ids);
 *   EMG_ROTATE: `rel` / `ld_rel` are the [cos | sin] image emg_eval_rel_rotate_image makes of the phase table (once per
 *               evaluation: the sincosf of emg_eval_build_queries, taken once per relation and coordinate);
 *   excl_ptr int64[n_rows + 1] / excl_idx int32: CSR of relation ids per row, ASCENDING within a row; both may be NULL.
 * One launch each, asynchronous on `stream`; no host read, no allocation.  EMG_EINVAL: unknown model / link, bad sizes or
 * strides, odd k_int of a complex model.  These symbols are additions: EMG_ABI_VERSION stays 9. */
/* RotatE's relation operand of EmbeddingModel.py:1856-1866's scoring on the relation side: img[r] = [cos(rel[r]) | sin(rel[r])],
 * k_int / 2 columns each, ld_img >= k_int. */
int emg_eval_rel_rotate_image(const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float* img, int64_t ld_img,
                              void* stream);
/* Counts of EmbeddingModel.py:1856-1866's scoring on the relation side, compared as :2010-2033 compares: with
 * I(row, r) = (int)(score * 1e5f) (link != EMG_LINK_LINEAR: the comparison integer THROUGH the link, as emg_eval_count_link) the
 * call writes, per row, over EVERY candidate relation (the true one included)
 *   cnt_gt = #{r : I > pos_int[row]}, cnt_eq = #{r : I == pos_int[row]}, and fcnt_gt / fcnt_eq: the same over the candidates
 * that are in the row's exclusion list — from the same scores, a membership test, not a second scoring pass.
 * pos_int int32[n_rows]: what emg_eval_build_queries (or its _link form) returns for EMG_EVAL_O on the same triples. */
int emg_eval_rel_count(int model, int32_t link, const float* ent, int64_t n_ent, int64_t ld_ent,
                       const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale,
                       const int32_t* test, int64_t n_rows, const int32_t* pos_int,
                       const int32_t* cand_rel, int64_t n_cand,
                       const int64_t* excl_ptr, const int32_t* excl_idx,
                       int32_t* cnt_gt, int32_t* cnt_eq, int32_t* fcnt_gt, int32_t* fcnt_eq, void* stream);
/* The scores of EmbeddingModel.py:1856-1866's scoring on the relation side, written out: S[row * lds + j] = score of
 * (s_row, candidate j, o_row), float, lds >= n_cand. */
int emg_eval_rel_scores_dense(int model, const float* ent, int64_t n_ent, int64_t ld_ent,
                              const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale,
                              const int32_t* test, int64_t n_rows, const int32_t* cand_rel, int64_t n_cand,
                              float* S, int64_t lds, void* stream);
/* Top-N of EmbeddingModel.py:1856-1866's scoring on the relation side: per row of the dense scores S (emg_eval_rel_scores_dense)
 * the top_n best candidates outside the row's exclusion list, in the total order of emg_eval_topn (higher score first; -0 == +0;
 * NaN last; equal scores by ascending relation id), ids int32 / scores float [n_rows, top_n], padded with (-1, -inf).
 * 1 <= top_n <= EMG_TOPN_MAX. */
int emg_eval_rel_topn(const float* S, int64_t lds, int64_t n_rows, int64_t n_cand, const int32_t* cand_rel,
                      const int64_t* excl_ptr, const int32_t* excl_idx, int32_t top_n,
                      int32_t* ids, float* scores, void* stream);

/* f32 -> bf16 (round-to-nearest-even) copy of a table for precision mode 1 */
int emg_to_bf16(const float* src, int64_t n_rows, int64_t ld_src, int32_t k_int,
                void* dst_bf16, int64_t ld_dst, void* stream);

/* ---- bf16 MFMA variant of the 1-vs-all path (DistMult / ComplEx / HolE only; v_mfma_f32_32x32x16_bf16).
 * Throughput mode, NOT a parity mode: operands are the bf16 (RNE) copies made by emg_to_bf16; the kernels
 * multiply over k_pad = round_up(k_int, 16) elements (one MFMA k-step) and rows are stored zero-padded
 * with ld >= round_up(k_pad, 64).  emg_eval_pos_int_bf16 writes the true entity of each row (self_ent) and the
 * positive's comparison integer computed by the SAME MFMA arithmetic as the count pass, so the true entity
 * counts as exactly one tie (as in the f32 path); emg_eval_filter_count_bf16 counts a filter list's self entry
 * as that same tie by index, so the filtered rank's self-cancellation stays exact, and scores every other filter
 * entry through the same MFMA k-step sequence as the count pass (32 (row, entity) pairs on the diagonal of one
 * 32x32 product), so a filter entity is subtracted with exactly the comparison result it was counted with.
 * ent_offset: global id of row 0 of `ent_bf16` (slabs); cand: optional row indices. */
int emg_eval_pos_int_bf16(int model, const void* ent_bf16, int64_t ld_ent, int32_t k_int, float scale,
                          const int32_t* test_spo, int64_t n_q, int side_mode, const void* q_bf16, int64_t ldq,
                          int32_t* pos_int, int32_t* self_ent, void* stream);
int emg_eval_count_bf16(int model, const void* q_bf16, int64_t ldq, const int32_t* pos_int, const int32_t* self_ent,
                        int64_t n_rows, const void* ent_bf16, int64_t n_cand, int64_t ld_ent, const int32_t* cand,
                        int64_t ent_offset, int32_t k_pad, float scale, int32_t* cnt_gt, int32_t* cnt_eq,
                        int32_t need, void* stream);
/* need: 0 = both counters (cnt_gt += #(>), cnt_eq += #(==));  1 = cnt_gt += #(>=) — all the 'worst' strategy
 * (the reference's default) reads;  2 = cnt_gt += #(>) — all 'best' reads.  With need != 0 the register-stationary
 * kernel does one comparison per score instead of two and the content of cnt_eq is unspecified. */
int emg_eval_filter_count_bf16(int model, const void* q_bf16, int64_t ldq, const int32_t* pos_int,
                               const int32_t* self_ent, int64_t n_rows, const void* ent_bf16, int64_t n_local,
                               int64_t ld_ent, int64_t ent_offset, int32_t k_int, float scale,
                               const int64_t* filt_ptr, const int32_t* filt_idx, int32_t* fcnt_gt,
                               int32_t* fcnt_eq, void* stream);
/* f32 -> IEEE half (round-to-nearest-even) copy of a table / query matrix for precision mode 2; same layout rules
 * as emg_to_bf16 (rows zero-padded to ld_dst >= round_up(k_int, 64)) */
int emg_to_f16(const float* src, int64_t n_rows, int64_t ld_src, int32_t k_int, void* dst_f16, int64_t ld_dst, void* stream);
/* The prefilter's error band.  With q~ = q + dq, e~ = e + de the half-rounded operands:
 *   |MFMA(q~, e~) - chain(q, e)| <= ||dq|| max||e~|| + ||q|| max||de|| + g (||q~|| max||e~|| + ||q|| max||e||),  g = 2 (k + 32) 2^-24
 * (Cauchy-Schwarz on dq.e~ + q.de, plus the accumulation error of either sum).  emg_eval_prefilter_bounds writes
 * bounds3 = (max||e||, max||e~||, max||e~ - e||) over the rows of a table (slab) and its half copy — float64, DEVICE memory;
 * emg_eval_prefilter_band evaluates the bound per query row from the ACTUAL residual norms of this query tile, inflated
 * by 1e-6 and rounded up to float: the `band` input of emg_eval_prefilter_f16. */
int emg_eval_prefilter_bounds(const float* ent, int64_t n_rows, int64_t ld_ent, const void* ent_f16, int64_t ld_f16,
                              int32_t k_int, double* bounds3, void* stream);
int emg_eval_prefilter_band(const float* q, int64_t n_rows, int64_t ldq, const void* q_f16, int64_t ldq_f16,
                            int32_t k_int, const double* bounds3, float* band, void* stream);

/* ---- exact ranks at MFMA speed (precision mode 2): half-precision MFMA prefilter (v_mfma_f32_32x32x16_f16: 11
 * significant bits, an 8x narrower error band than bf16 at the same rate) + exact re-scoring of the undecided.
 * `band[r]` is a rigorous upper bound, for query row r and EVERY candidate, on |accumulator of the f16 kernel -
 * accumulator of the exact f32 chain| (the host derives it from the rounding residuals of the operands, see
 * emgraph_amd/evaluation/ranking.py::prefilter_band).  emg_eval_prefilter_f16 adds to cnt_gt the candidates that
 * beat the positive by more than the band, drops those that lose by more than it, and writes the rest as
 * (row << 32 | global entity id) into `pairs`: the buffer is cut into emg_eval_prefilter_segments(n_rows, n_cand)
 * segments of pairs_capacity / segments entries, one per wave of the kernel (no atomics); pair_count[s] = entries
 * written to segment s, pair_count[segments] != 0 if some wave ran out of room (then the caller must use
 * emg_eval_count for these rows instead).  pair_count (uint32 [segments + 1]) is zeroed by the call.
 * Round 6 (ABI unchanged): with at least 2048 entries per segment (64 per entity tile of the chunk) the kernel first writes each
 * segment's undecided candidates as a BITMAP into the segment itself (64 lanes x 8 bytes per tile, branch-free) and a second
 * launch inside the same call turns every segment's bitmap into its pairs in place, entity tiles ascending; a segment with more
 * undecided candidates than entries is then recorded with pair_count[s] = 0 (its words stay a bitmap) beside the overflow flag.
 * What the caller sees after the call is as before; smaller segments take the emitting kernel (EMG_PRE_BITMAP=0 forces it).
 * EMG_ENOSUP for
 * shapes the register-stationary kernel does not cover.  emg_eval_rescore_pairs scores the pairs with the parity
 * path's arithmetic (k-ordered fmaf chain, int32(score*1e5)) and adds them to cnt_gt / cnt_eq, reading the counts
 * on the device (no host round trip between the two calls).  The resulting counters equal
 * emg_eval_count(precision 0) bit for bit. */
int64_t emg_eval_prefilter_segments(int64_t n_rows, int64_t n_cand);   /* = emg_eval_prefilter_segments_k(.., 400) */
/* Above 400 contraction columns (ComplEx / HolE k > 200, DistMult k > 400; up to emg_eval_prefilter_max_cols() = 800) the
 * prefilter runs as 4 waves x 128 query rows per workgroup — one wave per SIMD, whose 512 registers hold up to 50 query
 * fragments — instead of 8 x 256: the segment count depends on the width, and emg_eval_prefilter_waves(k_cols) (8 or 4)
 * is the segments_per_block of the re-scoring call. */
int64_t emg_eval_prefilter_segments_k(int64_t n_rows, int64_t n_cand, int32_t k_cols);
int32_t emg_eval_prefilter_waves(int32_t k_cols);
int32_t emg_eval_prefilter_max_cols(void);
/* row stride (elements, zero padded) the half-precision prefilter wants of BOTH operands for a contraction over k_cols
 * columns: the kernel is instantiated for 4, 7, 8, 10, 13, 16, 19, 22, 25 (8 waves) and 32, 38, 44, 50 (4 waves) k-steps
 * of 16 and fetches entity rows 64 columns at a time; a width in between runs the next instantiation over the zero
 * padding (k_cols <= 800) */
int64_t emg_eval_prefilter_ld(int32_t k_cols);
int emg_eval_prefilter_f16(int model, const void* q_f16, int64_t ldq, const int32_t* pos_int, const float* band,
                           int64_t n_rows, const void* ent_f16, int64_t n_cand, int64_t ld_ent, int64_t ent_offset,
                           int32_t k_pad, float scale, int32_t* cnt_gt, uint64_t* pairs, uint32_t* pair_count,
                           int64_t pairs_capacity, void* stream);
/* The same pass PROVING TIES (ABI 8, round 6).  The reference compares int32(score * 1e5) (EmbeddingModel.py:2010-2014): on a table
 * whose scores are small against 1e-5 — a freshly initialised model, the first epochs of a fit — every candidate ties with the
 * positive, and emg_eval_prefilter_f16 calls every tie undecided (its accumulator lies between the `>` and the `>=` threshold).
 * Here a candidate whose accumulator lies inside the positive's integer cell by more than the band is counted into cnt_eq, one
 * above it into cnt_gt, and only the two bands around the cell's ends are written as pairs.  With a band wider than the cell
 * (scores of order one) the result is emg_eval_prefilter_f16's.  Eight instead of four VALU instructions per score: for tables the
 * plain form cannot decide.  Needs segments that hold the bitmap form (pairs_capacity / segments >= 2048 at 32 tiles per chunk:
 * EMG_EINVAL otherwise); cnt_gt / cnt_eq as emg_eval_rescore_pairs continues them. */
int emg_eval_prefilter_f16_ties(int model, const void* q_f16, int64_t ldq, const int32_t* pos_int, const float* band,
                                int64_t n_rows, const void* ent_f16, int64_t n_cand, int64_t ld_ent, int64_t ent_offset,
                                int32_t k_pad, float scale, int32_t* cnt_gt, int32_t* cnt_eq, uint64_t* pairs,
                                uint32_t* pair_count, int64_t pairs_capacity, void* stream);
int emg_eval_rescore_pairs(int model, const float* Q, int64_t ldq, const int32_t* pos_int, const float* ent,
                           int64_t ld_ent, int64_t ent_offset, int32_t k_int, float scale, const uint64_t* pairs,
                           int64_t pairs_capacity, const uint32_t* pair_count, int64_t n_segments, int32_t* cnt_gt,
                           int32_t* cnt_eq, void* stream);
/* the same with the number of segments each workgroup of the prefilter wrote (8: emg_eval_prefilter_f16[_thr], 4:
 * emg_eval_prefilter_sad and the plain call): the re-scoring then runs each workgroup's segments on the XCD that produced
 * them, in the same order, so the entity rows of a chunk are re-read from that XCD's L2 instead of HBM */
int emg_eval_rescore_pairs_ex(int model, const float* Q, int64_t ldq, const int32_t* pos_int, const float* ent,
                              int64_t ld_ent, int64_t ent_offset, int32_t k_int, float scale, const uint64_t* pairs,
                              int64_t pairs_capacity, const uint32_t* pair_count, int64_t n_segments,
                              int32_t segments_per_block, int32_t* cnt_gt, int32_t* cnt_eq, void* stream);
/* the same, told how many consecutive query rows a segment covers (32: the waves of emg_eval_prefilter_f16[_thr]; 0: not
 * known): segments of >= 512 pairs are then re-scored by one workgroup each with the segment's query rows held in LDS */
int emg_eval_rescore_pairs_rows(int model, const float* Q, int64_t ldq, const int32_t* pos_int, const float* ent,
                                int64_t ld_ent, int64_t ent_offset, int32_t k_int, float scale, const uint64_t* pairs,
                                int64_t pairs_capacity, const uint32_t* pair_count, int64_t n_segments,
                                int32_t segments_per_block, int32_t rows_per_segment, int32_t* cnt_gt, int32_t* cnt_eq,
                                void* stream);
/* ---- ranking THROUGH the score link (embedding_model_params 'non_linearity'; EMG_LINK_* above) ----
 * The reference applies the link to the positive's score and to every corruption's score (EmbeddingModel.py:1868-1879) and
 * perform_comparision then compares int32(phi(score) * 1e5) (:2010-2033).  The calls below are the exact (precision 0) calls above
 * with that comparison integer: cmp = int32(phi(score) * 1e5), phi = the link with the SAME bits the training step and
 * emg_link_scores produce (one formula in the library).  link: EMG_LINK_LINEAR .. EMG_LINK_SOFTPLUS, anything else EMG_EINVAL;
 * EMG_LINK_LINEAR is the plain call (which forwards here).  All six models.  A saturating link makes ties of whole stretches
 * of the score axis (tanh(s) * 1e5 truncates to 99999 for every s above ~6.1): cnt_eq counts them, as the reference does.
 * These symbols are additions: EMG_ABI_VERSION stays 9, no existing structure or entry point changes. */
/* emg_eval_build_queries with pos_int = int32(phi(score_pos) * 1e5) (EmbeddingModel.py:1865-1879, 2010-2014); Q is the same */
int emg_eval_build_queries_link(int model, int32_t link, const float* ent, int64_t n_ent, int64_t ld_ent,
                                const float* rel, int64_t n_rel, int64_t ld_rel, int32_t k_int, float scale,
                                const int32_t* test_spo, int64_t n_q, int side_mode,
                                float* Q, int64_t ldq, int32_t* pos_int, void* stream);
/* emg_eval_count (precision must be 0) comparing through the link (EmbeddingModel.py:1868-1879, 2010-2033) */
int emg_eval_count_link(int model, int32_t link, const float* Q, int64_t ldq, const int32_t* pos_int, int64_t n_rows,
                        const float* ent, int64_t n_cand, int64_t ld_ent, const int32_t* cand,
                        int32_t k_int, float scale, int precision, int32_t* cnt_gt, int32_t* cnt_eq, void* stream);
/* emg_eval_filter_count comparing through the link (EmbeddingModel.py:1942-1963 on the linked scores of :1868-1879) */
int emg_eval_filter_count_link(int model, int32_t link, const float* Q, int64_t ldq, const int32_t* pos_int, int64_t n_rows,
                               const float* ent, int64_t n_local, int64_t ld_ent, int64_t ent_offset,
                               int32_t k_int, float scale, int precision,
                               const int64_t* filt_ptr, const int32_t* filt_idx,
                               int32_t* fcnt_gt, int32_t* fcnt_eq, void* stream);
/* emg_eval_rescore_pairs_rows comparing through the link (EmbeddingModel.py:1856-1879, 2010-2033): the segment forms only */
int emg_eval_rescore_pairs_link(int model, int32_t link, const float* Q, int64_t ldq, const int32_t* pos_int, const float* ent,
                                int64_t ld_ent, int64_t ent_offset, int32_t k_int, float scale, const uint64_t* pairs,
                                int64_t pairs_capacity, const uint32_t* pair_count, int64_t n_segments,
                                int32_t segments_per_block, int32_t rows_per_segment, int32_t* cnt_gt, int32_t* cnt_eq,
                                void* stream);
/* Exact-fast mode (the half-precision MFMA prefilter) under a link, contraction models (DESIGN.md 4.2 "Ranking through a link").
 * c(x) = int32(phi(x) * 1e5) over the ordered non-NaN floats x_0 < x_1 < ... (-inf first, +inf last, -0 before +0).
 * emg_eval_link_order_w: the committed order slack W of a link — c(x_i) <= c(x_j) whenever j - i >= W, the smallest of
 *   {1, 2, 4, 8, 16, 32} an exhaustive sweep found (libm's tanhf / expf / logf are not promised monotone); 1 for the linear
 *   link; 0: no W up to 32 holds, the link is ranked by the exact kernel only; -1: unknown link.
 * emg_eval_link_order_violations: the sweep.  *count (device, uint64; written, not accumulated) = the number of (i, d) with
 *   x_i in [lo, hi] (given as IEEE bit patterns, inclusive, not NaN, lo <= hi), d in [W, 2W), x_(i+d) <= +inf and
 *   c(x_i) > c(x_(i+d)); every gap >= W is a sum of gaps in [W, 2W), so zero over all floats (lo = 0xff800000, hi = 0x7f800000)
 *   proves the property.  1 <= W <= 32.  link | 0x100 (tests only): c negated, so that every step of c is a violation.
 * emg_eval_link_thresholds: per query row with positive integer p = pos_int[row], by bisection (valid under the property):
 *   a with c(x_a) <= p < c(x_(a+1)), b with c(x_b) < p <= c(x_(b+1)); then in the score domain
 *     G_out = x_(a+1+W): x >= G_out is greater for certain;   E_out = x_(b-W): x <= E_out is smaller for certain;
 *     G_in = x_(a-W), E_in = x_(b+1+W):  E_in <= x <= G_in is a tie for certain;  everything else is undecided.
 *   Where an invariant cannot be set up at -inf / +inf there is no edge: +inf stands for "nothing is greater" / "everything is
 *   smaller", -inf for "nothing is smaller" / "everything is greater".  thr_score [4 n_rows] = G_out | E_out | G_in | E_in
 *   (may be NULL).  thr [2 n_rows] (the convention of emg_eval_prefilter_f16_thr) and thr4 [4 n_rows] (for
 *   emg_eval_prefilter_f16_thr4) are the same thresholds in the ACCUMULATOR domain (score = fl(acc * scale); scale = 1 except
 *   HolE), widened outwards — the tie zone inwards — by band[row] + 1e-6 |t| + 1e-30 as the prefilter widens its own; a row
 *   whose band is not below 1e30 is all-undecided.  Either may be NULL; band may be NULL if both are.  EMG_ENOSUP for a link
 *   whose W is 0.  Replaces, for the prefilter, the comparison of EmbeddingModel.py:1868-1879 + 2010-2033.
 * emg_eval_prefilter_f16_thr4: emg_eval_prefilter_f16_ties with all four accumulator thresholds given (thr4 [4 n_rows]:
 *   counted into cnt_gt when acc >= thr4[r]; smaller when acc < thr4[n_rows + r]; counted into cnt_eq when
 *   thr4[3 n_rows + r] <= acc < thr4[2 n_rows + r]; else emitted).  Same bitmap-segment requirement. */
int32_t emg_eval_link_order_w(int32_t link);
int emg_eval_link_order_violations(int32_t link, int32_t W, uint32_t lo_bits, uint32_t hi_bits, uint64_t* count, void* stream);
int emg_eval_link_thresholds(int32_t link, const int32_t* pos_int, const float* band, int64_t n_rows, float scale,
                             float* thr, float* thr4, float* thr_score, void* stream);
int emg_eval_prefilter_f16_thr4(const void* q_f16, int64_t ldq, const float* thr4, int64_t n_rows, const void* ent_f16,
                                int64_t n_cand, int64_t ld_ent, int64_t ent_offset, int32_t k_pad, int32_t* cnt_gt,
                                int32_t* cnt_eq, uint64_t* pairs, uint32_t* pair_count, int64_t pairs_capacity, void* stream);
/* ENTITY-TILE-MAJOR form of the re-scoring (round 5): the undecided pairs of all segments are bucketed by tile of 32 entity rows
 * (histogram | scan | scatter into `sorted`, capacity >= pairs_capacity), then one workgroup per tile holds the tile's f32 rows in
 * LDS and streams the query rows of its pairs — the query matrix of a call fits L2 / MALL where the entity table does not.  Same
 * chain and comparison as emg_eval_rescore_pairs; n_local = rows of `ent`; tile_ws: emg_eval_rescore_tiles_ws_bytes(n_local)
 * bytes, ZERO before its first use (the call leaves it zero).  EMG_ENOSUP for rows that are not 16-byte aligned or whose
 * 32-row image does not fit LDS: use emg_eval_rescore_pairs_rows.  Replaces the same reference lines as emg_eval_rescore_pairs
 * (EmbeddingModel.py:1856-1866, 2010-2033). */
int64_t emg_eval_rescore_tiles_ws_bytes(int64_t n_local);
int emg_eval_rescore_pairs_tiles(int model, const float* Q, int64_t ldq, const int32_t* pos_int, const float* ent,
                                 int64_t ld_ent, int64_t ent_offset, int64_t n_local, int32_t k_int, float scale,
                                 const uint64_t* pairs, int64_t pairs_capacity, const uint32_t* pair_count, int64_t n_segments,
                                 uint64_t* sorted, int64_t sorted_capacity, void* tile_ws, int64_t tile_ws_bytes,
                                 int32_t* cnt_gt, int32_t* cnt_eq, void* stream);
int emg_eval_scores_dense_bf16(int model, const void* q_bf16, int64_t ldq, int64_t n_rows, const void* ent_bf16,
                               int64_t n_cand, int64_t ld_ent, const int32_t* cand, int32_t k_pad, float scale,
                               float* S, int64_t lds, void* stream);

/* TransE-L2 through the same half-precision MFMA prefilter: ||q - e||^2 = |q|^2 - (2 q.e - |e|^2) is a contraction over
 * k_int + 2 coordinates, q' = [2q | -1 | -1], e' = [e | n_hi | n_lo], n_hi + n_lo ~ |e|^2 (TransE.py:208-216 with norm 2:
 * score = -sqrt(sum_k (q_k - e_k)^2), compared as int(score * 1e5), EmbeddingModel.py:2010-2033).
 *   emg_to_f16_l2            f32 rows -> half rows of ld_dst >= k_int + 2 columns.  is_query = 0: [e | n_hi | n_lo | 0..],
 *                            *n_residual_max (device double, optional, written by the call) = max |n_hi + n_lo - |e|^2|;
 *                            is_query = 1: [2q | -1 | -1 | 0..] and, if `doubled` is given, the f32 rows 2q (ld_src stride)
 *   emg_eval_l2_thresholds   per query row the two accumulator thresholds (thr float [2 * n_rows]) from pos_int, the
 *                            band of emg_eval_prefilter_band(2q, half(2q)) and bounds4 = the three norms of
 *                            emg_eval_prefilter_bounds followed by *n_residual_max
 *   emg_eval_prefilter_f16_thr  emg_eval_prefilter_f16 with the thresholds given instead of derived from pos_int / band:
 *                            cnt_gt[row] += #(acc >= thr[row]); pairs with thr[n_rows + row] <= acc < thr[row] are emitted
 * followed by emg_eval_rescore_pairs(EMG_TRANSE_L2, ...): the counters equal emg_eval_count's bit for bit. */
int emg_to_f16_l2(const float* src, int64_t n_rows, int64_t ld_src, int32_t k_int, int is_query, void* dst_f16,
                  int64_t ld_dst, float* doubled, double* n_residual_max, void* stream);
int emg_eval_l2_thresholds(const float* Q, int64_t n_rows, int64_t ldq, const int32_t* pos_int, const float* band,
                           const double* bounds4, int32_t k_int, float* thr, void* stream);
int emg_eval_prefilter_f16_thr(const void* q_f16, int64_t ldq, const float* thr, int64_t n_rows, const void* ent_f16,
                               int64_t n_cand, int64_t ld_ent, int64_t ent_offset, int32_t k_pad, int32_t* cnt_gt,
                               uint64_t* pairs, uint32_t* pair_count, int64_t pairs_capacity, void* stream);

/* TransE-L1: the ranks of emg_eval_count, bit for bit, at integer speed (csrc/emg_rank_sad.hip).  The score of the
 * reference, -sum_k |q_k - e_k| (TransE.py:208-216 with norm 1, compared as int(score * 1e5), EmbeddingModel.py:
 * 2010-2033), is bounded from both sides by a sum of absolute differences of 16-bit fixed-point images of the rows
 * (v_sad_u16: two coordinates per instruction); candidates the bound decides are counted, the rest re-scored by
 * emg_eval_rescore_pairs (which takes TransE model ids for this purpose).
 *   emg_eval_sad_range      range[0] = max|ent|, range[1] = max|rel| (device doubles, written by the call): the image
 *                           maps [-R, R], R = (range[0] + range[1])(1 + 1e-6), onto 0..65535 — every query row
 *                           emg_eval_build_queries makes from these tables (s+p, o-p) lies inside
 *   emg_eval_sad_ld         columns of an image row for k_int coordinates (k_int rounded up to 16)
 *   emg_eval_sad_quantize   f32 rows -> u16 image rows (ld_dst u16 columns, padding columns 0)
 *   emg_eval_sad_thresholds per query row the integer sums below which a candidate certainly compares greater (lo)
 *                           and above which certainly less (hi) than pos_int
 *   emg_eval_prefilter_sad  cnt_gt[row] += #(candidates with sum < lo); (row << 32 | ent_offset + column) of the
 *                           candidates with lo <= sum <= hi into `pairs`, cut into emg_eval_sad_segments(n_rows,
 *                           n_cand) segments exactly as emg_eval_prefilter_f16 does (pair_count zeroed by the call;
 *                           pair_count[segments] != 0: some wave ran out of room, use emg_eval_count for these rows) */
int emg_eval_sad_range(const float* ent, int64_t n_ent, int64_t ld_ent, const float* rel, int64_t n_rel, int64_t ld_rel,
                       int32_t k_int, double* range, void* stream);
int64_t emg_eval_sad_ld(int32_t k_int);
int emg_eval_sad_quantize(const float* src, int64_t n_rows, int64_t ld_src, int32_t k_int, const double* range,
                          void* dst_u16, int64_t ld_dst, void* stream);
int emg_eval_sad_thresholds(const int32_t* pos_int, int64_t n_rows, int32_t k_int, const double* range, uint32_t* lo,
                            uint32_t* hi, void* stream);
int64_t emg_eval_sad_segments(int64_t n_rows, int64_t n_cand);
int emg_eval_prefilter_sad(const void* q_u16, int64_t ldq, const uint32_t* lo, const uint32_t* hi, int64_t n_rows,
                           const void* ent_u16, int64_t n_cand, int64_t ld_ent, int64_t ent_offset, int32_t k_int,
                           int32_t* cnt_gt, uint64_t* pairs, uint32_t* pair_count, int64_t pairs_capacity, void* stream);

/* RotatE: the ranks of emg_eval_count(EMG_ROTATE), bit for bit, through a half-precision prefilter (csrc/emg_rank_rotate.hip;
 * DESIGN.md 4.5 "Exact-fast ranking" proves the band).  The score of the reference, -sum_j |q_j - e_j| over the complex
 * coordinates (compared as int(score * 1e5), EmbeddingModel.py:2010-2033), is bounded from both sides by the same sum over half
 * images of the rows; candidates the bound decides are counted, the rest re-scored by emg_eval_rescore_pairs (which takes
 * EMG_ROTATE for this purpose: linear link, the wave-per-segment form; EMG_ENOSUP under another link).
 *   emg_eval_rotate_ld        columns (halves) of an image row for k_int coordinates (k_int rounded up to 16)
 *   emg_eval_rotate_image     rows [re | im] of k_int floats (an entity table, or Q of emg_eval_build_queries), times `scale` (a
 *                             power of two in [1, 2^24]: exact) -> half image rows, (re_j, im_j) adjacent, padding columns 0,
 *                             values below 2^-14 written as 0; rho[row] = sum_j |x_j scale - image_j| (moduli of the complex
 *                             residuals, rounded up).  stats (3 device doubles, written by the call): [0] = max rho,
 *                             [1] = max |x| (unscaled), [2] != 0 iff an entry is not finite or |x scale| > 32752 (half of the
 *                             half range: every difference of two image values is finite).  img_f16 == NULL: the range pass
 *                             alone (rho may be NULL).  check != 0: the call reads stats back (it synchronises the stream) and
 *                             returns EMG_ENOSUP for a refused table — the caller takes emg_eval_count; check == 0: no host
 *                             read, emg_eval_rotate_thresholds reads the verdict on the device
 *   emg_eval_rotate_thresholds per query row the accumulator values below which a candidate certainly compares greater (lo)
 *                             and above which certainly less (hi) than pos_int, the whole band folded in; rho_q / q_stats: of
 *                             the query image, ent_stats: of the entity image (same scale).  A refused image on either side,
 *                             or a saturated pos_int, leaves every candidate of the row undecided (lo 0, hi +inf)
 *   emg_eval_prefilter_rotate cnt_gt[row] += #(candidates with accumulator < lo); (row << 32 | ent_offset + column) of the
 *                             candidates with lo <= accumulator <= hi into `pairs`, cut into
 *                             emg_eval_prefilter_rotate_segments(n_rows, n_cand) segments exactly as emg_eval_prefilter_sad
 *                             does (pair_count zeroed by the call; pair_count[segments] != 0: some wave ran out of room, use
 *                             emg_eval_count for these rows)
 *   emg_eval_prefilter_rotate_dense  the same arithmetic through the same device function, the accumulators divided by
 *                             `scale` as float A [n_rows, lda]: small sizes, for tests (the counterpart of emg_eval_scores_dense)
 * These symbols are additions: EMG_ABI_VERSION stays 9, no existing structure or entry point changes. */
int64_t emg_eval_rotate_ld(int32_t k_int);
int emg_eval_rotate_image(const float* src, int64_t n_rows, int64_t ld_src, int32_t k_int, float scale, void* img_f16,
                          int64_t ld_img, float* rho, double* stats, int32_t check, void* stream);
int emg_eval_rotate_thresholds(const int32_t* pos_int, const float* rho_q, int64_t n_rows, int32_t k_int, float scale,
                               const double* q_stats, const double* ent_stats, float* lo, float* hi, void* stream);
int64_t emg_eval_prefilter_rotate_segments(int64_t n_rows, int64_t n_cand);
int emg_eval_prefilter_rotate(const void* q_f16, int64_t ldq, const float* lo, const float* hi, int64_t n_rows,
                              const void* ent_f16, int64_t n_cand, int64_t ld_ent, int64_t ent_offset, int32_t k_int,
                              int32_t* cnt_gt, uint64_t* pairs, uint32_t* pair_count, int64_t pairs_capacity, void* stream);
int emg_eval_prefilter_rotate_dense(const void* q_f16, int64_t ldq, int64_t n_rows, const void* ent_f16, int64_t n_cand,
                                    int64_t ld_ent, int32_t k_int, float scale, float* A, int64_t lda, void* stream);

/* TYPED ranking (csrc/emg_rank_typed.hip): every query row counted against the candidate pool of ITS group, all groups in one
 * launch.  NOT in the reference, which ranks against all entities or one global list (EmbeddingModel.py:1856-1866, :1898-1940);
 * the precedents are LibKGE's type-constrained ranking and the local closed-world assumption of Krompass et al. 2015: the
 * candidates of (s, p, ?) are the entities observed as an object of p (its range), those of (?, p, o) its domain.
 *   Q, pos_int     the query rows and the positives' comparison integers of emg_eval_build_queries (linear link)
 *   row_group      int32 [n_rows]: the group of each row; < 0 or >= n_groups: the row is not counted here.  Rows of one group
 *                  should be consecutive (non-decreasing ids within each side is what the host passes): the kernel works on
 *                  runs of equal ids inside windows of 64 rows, any order is CORRECT, sorted rows make the fewest tiles
 *   pool_ptr       int64 [n_groups + 1], ascending from pool_ptr[0] >= 0; pool_idx int32 [pool_ptr[n_groups]]: the members of
 *                  group g are pool_idx[pool_ptr[g] .. pool_ptr[g + 1]), entity ids in [0, n_ent) (an id outside is skipped).
 *                  The host layout (emgraph_amd/type_constraints.py): g = 2 p + side, side 0 = domain (subject corrupted),
 *                  side 1 = range (object corrupted), ids ascending and distinct
 *   cnt_gt, cnt_eq int32 [n_rows], ACCUMULATED: += the members of the row's pool whose comparison integer int32(score * 1e5) is
 *                  > / == pos_int[row], the score being the canonical chain of emg_eval_count (every model id, EMG_ROTATE and
 *                  EMG_TRANSE_P with `scale` = the order included): what emg_eval_count(..., cand = that pool) adds for the row
 * An EMPTY group counts nothing: a caller for which "no pool" means "all entities" gives such rows a negative group and counts
 * them with emg_eval_count.  One launch, no workspace, no host read: workgroups take tiles of <= 64 consecutive rows of one group
 * x <= 64 members of its pool (LDS-tiled f32 VALU, rows gathered by id), work is sum_g rows_g |pool_g| rounded up to tiles.
 * EMG_EINVAL: unknown model, bad strides, odd k_int with EMG_ROTATE, n_ent or n_groups >= 2^31.
 * This symbol is an addition: EMG_ABI_VERSION stays 9, no existing structure or entry point changes. */
int emg_eval_count_grouped(int model, const float* Q, int64_t ldq, const int32_t* pos_int, int64_t n_rows,
                           const int32_t* row_group, const float* ent, int64_t n_ent, int64_t ld_ent,
                           const int64_t* pool_ptr, const int32_t* pool_idx, int64_t n_groups, int32_t k_int, float scale,
                           int32_t* cnt_gt, int32_t* cnt_eq, void* stream);

/* SAMPLED ranking (csrc/emg_rank_lists.hip): every query row counted against a candidate list of ITS OWN.  NOT in the reference,
 * which ranks against all entities or one global list (EmbeddingModel.py:1856-1866, :1898-1940); the precedents are OGB's
 * head_neg / tail_neg arrays (ogbl-wikikg2, ogbl-biokg), DGL-KE's neg_sample_size_eval and PyKEEN's SampledRankBasedEvaluator.
 *   Q, pos_int     the query rows and the positives' comparison integers of emg_eval_build_queries (linear link)
 *   cand           int32 [n_rows, ld_cand >= n_cand] entity ids: the candidates of row r are cand[r * ld_cand .. + n_cand).  An id
 *                  < 0 or >= n_ent is PADDING: never used as an index, never counted (ragged lists are padded with -1).  A
 *                  duplicate is a candidate each time it occurs (sampling with replacement)
 *   excl_ptr       int64 [n_rows + 1] / excl_idx int32, ascending within a row (the layout of the filter CSR of
 *                  emg_eval_filter_count); both may be NULL.  A candidate found in its row's range (bisection) is skipped: how
 *                  known positives and the row's own true entity are kept out, in the same launch
 *   cnt_gt, cnt_eq int32 [n_rows], ACCUMULATED: += the surviving candidates whose comparison integer int32(score * 1e5) is
 *                  > / == pos_int[row], the score being the canonical chain of emg_eval_count (every model id, EMG_ROTATE and
 *                  EMG_TRANSE_P with `scale` = the order, inf included): a pair has the bits emg_eval_scores_dense writes for it
 * One launch, no workspace, no host read: a wave takes one row and 64 candidates at a time, one lane per candidate; the candidate
 * rows are gathered in slices through the wave's LDS region with coalesced loads (16-byte aligned rows; others are read per lane).
 * n_rows == 0 or n_cand == 0: EMG_OK, nothing launched.
 * EMG_EINVAL: unknown model, bad strides (ldq, ld_ent < k_int, ld_cand < n_cand), odd k_int with EMG_ROTATE, a non-positive order
 * with EMG_TRANSE_P, n_ent >= 2^31, exactly one of excl_ptr / excl_idx NULL.
 *
 * emg_eval_draw_candidates fills such lists for the query rows of emg_eval_build_queries' row order (object-side rows first for
 * EMG_EVAL_SPO / EMG_EVAL_S_O): for the row of test triple g = q_offset + local index, side bit sd (1 = object side, 0 = subject
 * side) and column j,  o = philox4x32_10((uint32)g, (uint32)(g >> 32), (uint32)j, sd, (uint32)seed, (uint32)(seed >> 32)),
 * id = mulhi64((o.v[2] << 32) | o.v[1], n_ent) (corruption_draw's reduction).  Uniform with replacement, keyed by the triple's
 * position in the whole test set (the lists do not depend on how the set is cut into calls), blind to the graph: known positives
 * are dealt with by the exclusion of the count.  EMG_EINVAL: bad side_mode, n_ent outside [1, 2^31), ld_cand < n_cand.
 * These symbols are additions: EMG_ABI_VERSION stays 9, no existing structure or entry point changes. */
int emg_eval_count_lists(int model, const float* Q, int64_t ldq, const int32_t* pos_int, int64_t n_rows,
                         const float* ent, int64_t n_ent, int64_t ld_ent,
                         const int32_t* cand, int64_t ld_cand, int32_t n_cand,
                         const int64_t* excl_ptr, const int32_t* excl_idx,
                         int32_t k_int, float scale, int32_t* cnt_gt, int32_t* cnt_eq, void* stream);
int emg_eval_draw_candidates(int64_t n_q, int64_t q_offset, int side_mode, int32_t n_cand, int64_t n_ent,
                             uint64_t seed, int32_t* cand, int64_t ld_cand, void* stream);

/* ====================== shared negatives: chunks of positives scored against common draws (csrc/emg_shared.hip) ======================
 * Not in the reference (the negative sharing of DGL-KE's neg_chunk_size / PyTorch-BigGraph's chunked uniform
 * negatives).  A batch of B positives is cut into G = ceil(B / C) chunks of C consecutive rows (the last may be short); every
 * chunk has ONE draw per corruption slot m = sd * eta + j (side-major, then eta-major: the slot order of emg_loss), and every
 * positive of the chunk is scored against all eta_total = n_sides * eta draws of its chunk:
 *   chunk_codes int32 [eta_total * G]: entry m * G + g = replacement | keep_subject << 31, the code layout of emg_corrupt_codes —
 *     per side, the output of emg_corrupt_codes with B := G.  THE IDENTITY the rest follows from: the step is the ordinary step
 *     with  codes[m * B + i] = chunk_codes[m * G + i / C].
 * emg_shared_forward: scores_pos [B], scores_neg [eta_total * B] in emg_loss's layout (entry m * B + i).  Every score is the
 *   canonical f32 chain of csrc/emg_chain.hpp over the query row emg_eval_build_queries forms (keep_subject: the object-side query
 *   of (s, p) against the replacement; otherwise the subject-side query of (p, o)); the positive is the object-side query against
 *   its own object: the bits emg_eval_scores_dense(precision 0) writes for the same (query row, candidate), all seven models.
 *   A workgroup takes one chunk and a slice of its draws; rows pass through LDS in column blocks (16-byte row loads where the
 *   tables' rows are 16-byte aligned and the model's column count is a multiple of 4, scalar loads otherwise).
 * emg_shared_backward: the adjoint.  g_pos [B] / g_neg [eta_total * B] = dL/dscore in that layout.  Gradient rows, no atomics,
 *   sums in a fixed order (two runs give the same bits); a term is the f32 product the ordinary step stores as a gradient row, the
 *   sum over a row's terms is carried in double and rounded to f32 once:
 *     contrib_ent[i]                  dL/dE[s_i]: the positive's own term, then the draws that keep the subject in ascending m
 *     contrib_ent[B + i]              dL/dE[o_i]: the positive's own term, then the draws that keep the object in ascending m
 *     contrib_ent[2B + m * G + g]     dL/dE[replacement m of chunk g], summed over the chunk's positives in ascending i
 *     contrib_rel[i]                  dL/dR[p_i]: the positive's own term, then every draw in ascending m
 *   (2B + eta_total * G entity rows where the ordinary step writes (2 + eta_total) * B), row stride ldc; the same launch writes their
 *   destinations dest_ent [2B + eta_total * G] / dest_rel [B] — group with emg_group_dest, apply with emg_apply_grouped (or
 *   emg_apply_rows).  raw_pos / raw_neg: the RAW scores emg_shared_forward wrote (before any emg_link_scores): required for
 *   EMG_TRANSE_L2 and EMG_TRANSE_P (the norm of a triple is minus its score), ignored otherwise.  The gradient formulas are those
 *   of emg_train_backward_ex(fused_loss = -1).
 * 1 <= C <= 256.  B == 0: EMG_OK, nothing launched.  EMG_EINVAL: C out of range, unknown model, bad strides, odd k_int with a
 * complex model, a null pointer, raw scores missing for a norm model, more draws per chunk than a workgroup's LDS holds (the
 * backward stages all eta_total replacement rows of a chunk: 3 C + eta_total <= 1500).  EMG_ENOSUP: emg_shared_backward with
 * EMG_TRANSE_P of infinite order.  These symbols are additions: EMG_ABI_VERSION stays 9, no existing structure or entry point changes. */
typedef struct emg_shared_args {
    int32_t model; int32_t k_int; float scale; int32_t eta_total;
    const float* ent; int64_t n_ent; int64_t ld_ent;
    const float* rel; int64_t n_rel; int64_t ld_rel;
    const int32_t* pos; int64_t B; int32_t C; int32_t reserved0;
    const int32_t* chunk_codes;
    float* scores_pos; float* scores_neg;               /* forward: out */
    const float* g_pos; const float* g_neg;             /* backward: dL/dscore */
    const float* raw_pos; const float* raw_neg;         /* backward: raw scores (norm models) */
    float* contrib_ent; float* contrib_rel; int64_t ldc;
    int32_t* dest_ent; int32_t* dest_rel;
} emg_shared_args;
int emg_shared_forward(const emg_shared_args* args, void* stream);
int emg_shared_backward(const emg_shared_args* args, void* stream);

/* ====================== relation negatives: the relation of a positive replaced (csrc/emg_relneg.hip) ======================
 * Not in the reference (PyKEEN's corruption_scheme ('h', 'r', 't'), LibKGE's num_samples.p, OpenKE's neg_rel).
 * Draw j of positive i = (s, p, o) is the triple (s, p', o):
 *   codes int32 [eta * B]: entry j * B + i = idx in [0, n_rel - 1) — emg_corrupt_codes' own draw with n_choices = n_rel - 1, no
 *     entity list, the side forced (the keep_subject bit is unused and zero);  p' = idx + (idx >= p): never the positive itself,
 *     uniform over the other n_rel - 1 relations.  The shift is made here, from `pos`.
 * emg_relneg_forward: scores_neg [eta * B], entry j * B + i = the score of (s_i, p'_ji, o_i) (a block of emg_loss's scores_neg);
 *   scores_pos [B] (may be NULL) = the score of the positive.  Every score has the bits emg_eval_rel_scores_dense writes for the
 *   same (pair, relation): the object-side query of (s, p') built per coordinate, then the canonical f32 chain of csrc/emg_chain.hpp
 *   against the object row, k ascending, one lane per chain; every model id of that entry point (EMG_SIMPLE and EMG_ROTATE — whose
 *   relation rows are phases HERE, not the [cos | sin] image — included).  A workgroup takes a run of positives; their s / o rows
 *   pass through LDS in column slices (16-byte row loads where the tables' rows are 16-byte aligned and the model's column count
 *   per half is a multiple of 4, scalar loads otherwise); a lane gathers its own relation row.
 * emg_relneg_backward: the adjoint.  g_neg [eta * B] (and g_pos [B], may be NULL) = dL/dscore.  Gradient rows, no atomics, a fixed
 *   summation order (two runs give the same bits).  A term is the f32 gradient row emg_train_backward_ex(fused_loss = -1, eta = 0)
 *   stores for the triple (s_i, p'_ji, o_i) taken as a positive under dL/dscore = g_neg[j * B + i]; a sum over terms is carried in
 *   double and rounded to f32 once.  With P = B if g_pos is given, else 0:
 *     contrib_ent[i]                dL/dE[s_i]: the positive's own term first (g_pos given), then draws j = 0 .. eta - 1
 *     contrib_ent[B + i]            the same for o_i
 *     contrib_rel[i]                dL/dR[p_i], the positive's own term — written only if g_pos is given
 *     contrib_rel[P + j * B + i]    dL/dR[p'_ji], one term
 *   row stride ldc; dest_ent [2 B] = (s | o), dest_rel [P + eta * B] = (p |) p' in the same layout — group with emg_group_dest,
 *   apply with emg_apply_grouped.  The eta * B relation rows are written past the caches (`nt`), the 2 B entity rows plainly
 *   (DESIGN.md 4.1 "Relation negatives").  raw_neg (and raw_pos with g_pos): the RAW scores of the triples (before any
 *   emg_link_scores): required for EMG_TRANSE_L2 and EMG_TRANSE_P (the norm of a triple is minus its score), ignored otherwise.
 * B == 0: EMG_OK, nothing launched.  EMG_EINVAL: n_rel < 2, eta < 1, an idx outside [0, n_rel - 1) (found by the kernel, which
 * never follows such an index: the call waits for its launch and reports it), bad strides, odd k_int of a complex model or of
 * EMG_SIMPLE, unknown model, a null pointer, raw scores missing for a norm model.  EMG_ENOSUP: emg_relneg_backward with EMG_TRANSE_P
 * of infinite order.  These symbols are additions: EMG_ABI_VERSION stays 9, no existing structure or entry point changes. */
typedef struct emg_relneg_args {
    int32_t model; int32_t k_int; float scale; int32_t eta;
    const float* ent; int64_t n_ent; int64_t ld_ent;
    const float* rel; int64_t n_rel; int64_t ld_rel;
    const int32_t* pos; int64_t B;
    const int32_t* codes;                               /* [eta * B], entry j * B + i = idx */
    float* scores_pos; float* scores_neg;               /* forward: out; scores_pos may be NULL */
    const float* g_pos; const float* g_neg;             /* backward: dL/dscore; g_pos may be NULL */
    const float* raw_pos; const float* raw_neg;         /* backward: raw scores (norm models) */
    float* contrib_ent; float* contrib_rel; int64_t ldc;
    int32_t* dest_ent; int32_t* dest_rel;
} emg_relneg_args;
int emg_relneg_forward(const emg_relneg_args* args, void* stream);
int emg_relneg_backward(const emg_relneg_args* args, void* stream);

/* ====================== batch-local Lp / N3 regulariser (csrc/emg_batchreg.hip) ======================
 * Not in the reference, whose LP regulariser penalises the full tables (LibKGE's regularize_weighted, PyKEEN's
 * LpRegularizer, the weighted nuclear 3-norm "N3" of Lacroix, Usunier, Obozinski, ICML 2018).  For the positives (s_i, p_i, o_i),
 * i < B, of a batch:
 *     R = sum_i [ lambda_ent (N(E[s_i]) + N(E[o_i])) + lambda_rel N(R[p_i]) ]            (every occurrence counted; a sum, not a mean)
 *   plain form    N(x) = sum_{c < k_int} |x_c|^p
 *   modulus form  N(x) = sum_{j < k} (x_j^2 + x_{j + k}^2)^(p / 2),  k = k_int / 2       (rows [re | im])
 * emg_batchreg, one launch: the gradient rows of R and their destinations, and R itself.
 *   coef_g_* = (float)(lambda p), coef_v_* = (float)lambda, rounded by the caller.  form_ent / form_rel: EMG_BATCHREG_PLAIN or
 *   EMG_BATCHREG_MODULUS, per table.
 *     contrib_ent[i]       lambda_ent dN/dx at E[s_i]
 *     contrib_ent[B + i]   the same at E[o_i]
 *     contrib_rel[i]       lambda_rel dN/dx at R[p_i] — written only if lambda_rel != 0 (coef_v_rel or coef_g_rel non-zero); otherwise
 *                          no relation rows and no relation destinations are produced, and rel / contrib_rel / dest_rel may be NULL
 *   row stride ldc; dest_ent [2 B] = (s | o), dest_rel [B] = p: emg_relneg_backward's layout — group with emg_group_dest, apply with
 *   emg_apply_grouped (a caller appends the rows behind a step's own).  The rows are stored plainly.
 *   Every operation is one correctly rounded f32 operation, nothing contracted.  The entry of coordinate w:
 *     plain    p = 1  coef_g * sign(w), sign(0) = 0       p = 2  coef_g * w       p = 3  coef_g * (|w| * w)
 *     modulus  (a, b) = (x_j, x_{j + k}), m = sqrtf(a * a + b * b); the entry of a (b alike):
 *              p = 1  coef_g * (a / m), 0 where m = 0     p = 2  coef_g * a       p = 3  coef_g * (m * a)
 *   value (a device double, may be NULL): R is ADDED to it.  The f32 terms |w|, w * w, (|w| * |w|) * |w| (plain, one per coordinate)
 *   and m, a * a + b * b, (m * m) * m (modulus, one per pair) are summed in double and scaled by (double)coef_v; one atomic per
 *   workgroup, so the association of the sum is free (a host compares at rtol 1e-12).
 *   16-byte accesses where every row is 16-byte aligned and the column count of a pass (the half width in the modulus form) is a
 *   multiple of 4, scalar ones otherwise.
 * B == 0: EMG_OK, nothing launched.  EMG_EINVAL: p outside 1..3, an unknown form, the modulus form with odd k_int, bad strides, a
 * null pointer, an id of `pos` outside its table (found by the kernel, which never follows such an id: the call waits for its launch
 * and reports it).  This symbol is an addition: EMG_ABI_VERSION stays 9, no existing structure or entry point changes. */
enum { EMG_BATCHREG_PLAIN = 0, EMG_BATCHREG_MODULUS = 1 };
typedef struct emg_batchreg_args {
    int32_t k_int; int32_t p;
    int32_t form_ent; int32_t form_rel;                 /* EMG_BATCHREG_* */
    float coef_g_ent; float coef_v_ent;                 /* (float)(lambda_ent p), (float)lambda_ent */
    float coef_g_rel; float coef_v_rel;
    const float* ent; int64_t n_ent; int64_t ld_ent;
    const float* rel; int64_t n_rel; int64_t ld_rel;
    const int32_t* pos; int64_t B;
    float* contrib_ent; float* contrib_rel; int64_t ldc;
    int32_t* dest_ent; int32_t* dest_rel;
    double* value;
} emg_batchreg_args;
int emg_batchreg(const emg_batchreg_args* args, void* stream);

/* ====================== one-call forms (compositions of the entry points above, one stream) ==============
 * The C-ABI sketched in SURVEY.md 8b.  A maintainer binding the library from the reference calls these once per
 * batch / per test set; the finer-grained entry points exist so that a host can overlap stages on several
 * streams (as emgraph_amd/training.py does). */

/* generate_corruptions_for_fit (protocol.py:531-659) in one call: out_spo int32 [B*eta, 3], eta-major.
 * entities_size > 0: replacements are ids drawn from [0, entities_size) (:616-619); otherwise they are drawn
 * from entities_list[0..n_list) (:620-641).  Draws: Philox4x32-10 keyed by (seed; row, counter). */
int emg_corrupt_fit(const int32_t* pos, int64_t B, int32_t eta, int side, int64_t entities_size,
                    const int32_t* entities_list, int64_t n_list, uint64_t seed, uint64_t counter,
                    int32_t* out_spo, void* stream);

/* Filtered ranks of n_q test triples against all entities (cand == NULL) or the rows cand[0..n_cand):
 * emg_eval_build_queries -> emg_eval_count[_bf16] -> emg_eval_filter_count[_bf16] -> rank assembly
 * (EmbeddingModel.py:1845-2033).  filt_ptr/filt_idx: optional CSR over the n_rows query rows in the row order
 * documented above (object-side rows first), GLOBAL entity ids, each list containing the row's true entity.
 * strategy: 0 worst | 1 best | 2 middle.  precision_mode: 0 exact f32 | 1 bf16 MFMA (statistical agreement) |
 * 2 the ranks of mode 0, bit for bit, through the half-precision MFMA prefilter + exact re-scoring (emg_to_f16,
 * emg_eval_prefilter_bounds / _band, emg_eval_prefilter_f16, emg_eval_rescore_pairs; one host synchronisation to read the
 * overflow flag; TransE-L1 goes through the 16-bit fixed-point prefilter emg_eval_prefilter_sad instead, TransE-L2
 * through the MFMA prefilter on the augmented rows of emg_to_f16_l2; the exact kernel takes over for candidate lists,
 * shapes the prefilter kernels do not cover and overflowing pair buffers — the pair buffer of a call is capped at
 * 1 GiB, so hand mode 2 a few thousand test triples per call (emgraph_amd/evaluation/ranking.py uses 4096): a much larger
 * call still returns the exact ranks, but through the exact kernel).
 * rank_out int32: [n_q] for side_mode 0,1,2; [n_q,2] = [subject_rank, object_rank] for side_mode 3. */
int emg_rank_1vsall(int model, const float* ent, int64_t n_ent, int64_t ld_ent, const float* rel, int64_t n_rel,
                    int64_t ld_rel, int32_t k_int, float scale, const int32_t* test_spo, int64_t n_q, int side_mode,
                    const int32_t* cand, int64_t n_cand, const int64_t* filt_ptr, const int32_t* filt_idx,
                    int strategy, int precision_mode, int32_t* rank_out, void* stream);

/* One training batch: corruptions of every side -> scores -> loss (accumulated into *loss_accum) -> gradients ->
 * row-sparse optimizer update of both tables (EmbeddingModel.py:614-822 + training/{sgd,momentum,adagrad,adam}.py), without the LP
 * regulariser.  `workspace` (device, emg_train_step_workspace_bytes) holds all per-batch scratch (since ABI 9 including
 * (1 + eta_total) * B floats for the unfused step's link factors, whether a link is set or not: one layout per shape).
 * inplace != 0: rows whose destination occurs once in the batch are updated by the gradient kernel itself. */
typedef struct emg_step_args {
    int32_t model; int32_t k_int; float scale; int32_t eta; int32_t n_sides; int32_t sides[4];
    float* ent; int64_t n_ent; int64_t ld_ent; float* rel; int64_t n_rel; int64_t ld_rel;
    float* ent_state0; float* ent_state1; float* rel_state0; float* rel_state1;   /* optimizer state, NULL if unused */
    int32_t* tag_ent; int32_t* tag_rel;                                           /* int32[n_rows], zeroed once */
    int32_t opt; int32_t step; float hyper[8];                                    /* as emg_apply_rows (hyper[6] = 0) */
    const int32_t* pos; int64_t B;                                                /* device int32 [B,3] */
    int64_t n_choices; const int32_t* entities_list; uint64_t seed; uint64_t draw_counter0;
    const int32_t* inj_mask; const int32_t* inj_repl;                             /* optional injected draws */
    int32_t loss; float margin; float alpha; double* loss_accum;
    int32_t inplace;
    void* workspace; int64_t workspace_bytes;
    int32_t link; float sw; const float* edge_w;   /* ABI 9: score link, structure weight, edge weights [B] (emg_backward_args) */
} emg_step_args;
int64_t emg_train_step_workspace_bytes(int64_t B, int32_t eta_total, int32_t k_int, int64_t n_ent, int64_t n_rel);
int emg_train_step(const emg_step_args* args, void* stream);

/* ====================== the training step as one call on several streams (emg_plan.hip) ======================
 * emg_train_step above is a single-stream composition.  A plan object additionally owns two high-priority side
 * streams (batch preparation of the NEXT batches runs there while the current one computes), a stream for the
 * relation table's apply, and the events between them, so that the multi-stream step emgraph_amd's fit() runs is
 * ONE library call per batch (EmbeddingModel.py:1388-1440 is the loop it stands for).  All buffers are the caller's;
 * the plan owns streams and events only.  Scratch is sized for cap_B positives per batch:
 *   scores, g : float [(1 + eta_total) * cap_B] each (only the unfused step — losses that couple a positive's
 *               negatives — uses them);  contrib_ent [(2 + eta_total) * cap_B, ldc], contrib_rel [cap_B, ldc];
 *   per slot  : codes int32 [eta_total * cap_B], dest_ent int32 [(2 + eta_total) * cap_B], dest_rel int32 [cap_B],
 *               single uint8 [(2 + eta_total) * cap_B], ws_* from emg_apply_workspace_bytes_ex.
 * n_slots = 1 + number of batches prepared ahead (0..2; 1 slot = everything on the caller's stream). */
typedef struct emg_plan_slot {
    int32_t* codes; int32_t* dest_ent; int32_t* dest_rel; uint8_t* single;
    void* ws_ent; int64_t ws_ent_bytes; void* ws_rel; int64_t ws_rel_bytes;
} emg_plan_slot;
typedef struct emg_plan_config {
    int32_t model; int32_t k_int; float scale; int32_t eta; int32_t n_sides; int32_t sides[4];
    float* ent; int64_t n_ent; int64_t ld_ent; float* rel; int64_t n_rel; int64_t ld_rel;
    float* ent_state0; float* ent_state1; float* rel_state0; float* rel_state1; int32_t* tag_ent; int32_t* tag_rel;
    int32_t opt; int32_t loss; float margin; float alpha;
    uint64_t seed; int64_t batches_count;            /* draw counter of (epoch, batch, side): see emg_prepare_args */
    const int32_t* X; int64_t n_triples;             /* the resident, id-mapped training set [n_triples, 3] */
    int64_t cap_B;
    float* scores; float* g; float* contrib_ent; float* contrib_rel; int64_t ldc;
    double* loss_accum; double* lp_sum;              /* lp_sum[2]: sum |w|^p of the entity / relation table */
    int32_t factored;                                /* 1: factored entity contributions (emg_prepare_args / emg_backward_args); contrib_ent then needs 4 * cap_B rows */
    int32_t loss_slots;                              /* loss_accum points to this many doubles (emg_backward_args.loss_slots; 0 / 1: one) */
    float lp_lambda_ent; float lp_lambda_rel; int32_t lp_p;   /* folded LP regulariser (0 = none; excludes inplace) */
    int32_t fused; int32_t inplace; int32_t normalize;   /* inplace: 0 off, 1 singletons in place, 2 the same through a stateful optimizer's
                                                            window form (emg_backward_args.inplace_window; with lr_t_hist: Adam's singleton
                                                            negatives replayed inside the scoring kernel, s / o slots through the apply) */
    int32_t n_slots; emg_plan_slot slots[4];
    int64_t aux_min_rows;                            /* ignored (both tables' applies are one launch) */
    void* ctl_buf; int64_t ctl_bytes;                /* optional device scratch (>= 32 * sizeof(emg_step_ctl)) for emg_plan_run */
    const float* lr_t_hist;                          /* != NULL (EMG_OPT_ADAM and / or LP): deferred dense pass (emg_deferred_catchup before every
                                                        scoring kernel, none afterwards); [s] = learning rate of step s (Adam: lr_t), filled
                                                        for every step the plan is given */
    /* ABI 9: score link and FocusE edge weights (emg_backward_args).  edge_w: float [n_triples], row i the weight of X's row i;
     * link_fac: float [(1 + eta_total) * cap_B] scratch, needed only where the step is not fused.  The structure weight is per
     * batch (emg_plan_batch.sw).  A plan with a link or edge weights trains through emg_plan_step; emg_plan_graph_ok says no. */
    int32_t link; int32_t reserved2; const float* edge_w; float* link_fac;
} emg_plan_config;
typedef struct emg_plan_batch {
    int64_t start; int64_t B; int32_t epoch; int32_t batch;   /* rows [start, start + B) of X; 1-based epoch / batch */
    int64_t n_choices; const int32_t* entities_list;           /* corruption pool (0 / NULL: all n_ent entities) */
    const int32_t* inj_mask; const int32_t* inj_repl;          /* optional injected draws */
    float sw; int32_t reserved0;                               /* ABI 9: structure weight of this batch (read with emg_plan_config.edge_w) */
} emg_plan_batch;
int emg_plan_create(const emg_plan_config* cfg, void** plan);
/* train on `cur`; `next[0..n_next)` (nearest first) are prepared ahead on the side streams if a slot is free.
 * step >= 1 is the optimizer step number, hyper6 = {lr, momentum, beta1, beta2, eps, lr_t} for it. */
int emg_plan_step(void* plan, const emg_plan_batch* cur, int32_t step, const float* hyper6,
                  const emg_plan_batch* next, int32_t n_next, void* stream);
/* The same steps as GRAPH replays (small batches: a step is shorter than its launches take to issue).  The step's
 * kernels are captured once per graph length (<= 32 steps) with their per-step values read from device records
 * (emg_step_ctl) that each call writes before the replay: two launches per 32 steps from the host.  batches[i] trains as
 * optimizer step first_step + i with hyper6s[6 i .. 6 i + 5]; results are those of n emg_plan_step calls.
 * emg_plan_graph_ok: 1 if the plan can (fused pair-local loss, 16-byte rows of more than 16 chunks, counting grouping,
 * ctl_buf given, linear link and no edge weights); injected draws need emg_plan_step. */
int emg_plan_graph_ok(void* plan);
/* 1 if a plan of this shape can DEFER its dense pass (emg_plan_config.lr_t_hist): emg_deferred_catchup walks the segment
 * descriptors of the counting grouping, which is chosen only while a table is not much longer than its batch has gradient
 * rows (n_rows <= 16 n + 2^20; EMG_GROUPING=sort forces the radix-sort backend).  emg_plan_create refuses lr_t_hist otherwise:
 * the caller keeps the dense pass (emgraph_amd/training.py::Trainer._make_plan). */
int emg_plan_deferred_ok(int64_t cap_B, int32_t eta_total, int64_t n_ent, int64_t n_rel);
int emg_plan_run(void* plan, const emg_plan_batch* batches, int32_t n, int32_t first_step, const float* hyper6s,
                 void* stream);
/* HIP-event timing of the next max_samples launches of every stage (0 = off); avg_ms / counts: 9 entries =
 * prepare, fused, forward, loss, backward, apply_ent, apply_rel, clip, catchup (the deferred pass's emg_deferred_catchup calls).
 * apply_ent times the one apply launch over both tables; apply_rel stays empty. */
int emg_plan_timing(void* plan, int32_t max_samples);
int emg_plan_stage_ms(void* plan, float* avg_ms, int32_t* counts);
int emg_plan_destroy(void* plan);

/* ====================== Platt-scaling calibration on frozen embeddings (emg_calib.hip) ======================
 * EmbeddingModel._calibrate / _predict_proba (EmbeddingModel.py:2212-2575; AmpliGraph 1.x's calibrate / predict_proba): two
 * scalars (w, b) fitted to the RAW scores (no link, no FocusE weight: :2245-2258, :2567-2569), logit x = -(w s + b),
 * loss = sum weight * ce(label, x) / #scores, ce(z, x) = max(x, 0) - x z + log1p(exp(-|x|)) (:2439-2506; the weights are those
 * of tf.losses.sigmoid_cross_entropy, which the reference's port dropped: DESIGN.md 0).  These symbols are additions:
 * EMG_ABI_VERSION stays 9, no existing structure or entry point changes.
 *
 * Every call is asynchronous on `stream`.  `workspace` (device, 16-byte aligned, emg_calib_ws_bytes) holds a ticket counter
 * and one slot of partial sums per workgroup: it must be ZERO before the first launch that uses it and is left re-armed by every
 * launch (no memset between launches); launches that share a workspace run on one stream. */

/* bytes of the workspace for emg_calib_step on a batch of n rows, or emg_calib_moments on n scores in all */
int64_t emg_calib_ws_bytes(int64_t n);

/* One optimiser step of the calibration WITHOUT negatives (:2212-2260, :2509-2531), one launch: row i of the batch draws its
 * corruption exactly as emg_corrupt_codes(B, 1, EMG_SIDE_SO, n_ent, NULL, seed, draw_counter, ...) draws row i (eta = 1, side
 * 's,o', over all entities: :2248-2255), the negative's rows are gathered and scored (bit-equal to emg_score_triples on the
 * materialised triple, all six model ids, any k_int), the logistic terms of the negative and of its positive (scores_pos[i],
 * scored once by the caller: the embeddings are frozen) are formed in double and summed in a fixed order, and the workgroup
 * that finishes last applies Keras Adam (adam.py:45: lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), x -= lr_t m / (sqrt(v) + eps))
 * to the state record:  state = {w, b, m_w, m_b, v_w, v_b, step, loss_sum} (doubles; step counts the launches, loss_sum
 * accumulates the batch losses).  The host neither reads nor writes anything between two steps.
 * dbg_neg int32 [B, 3] / dbg_scores float [B] (NULL in production): the negatives the draws imply and their scores. */
typedef struct emg_calib_args {
    int32_t model; int32_t k_int; float scale; int32_t reserved0;
    const float* ent; int64_t n_ent; int64_t ld_ent; const float* rel; int64_t n_rel; int64_t ld_rel;
    const int32_t* pos; int64_t B;                 /* the batch: device int32 [B, 3] */
    const float* scores_pos;                       /* float [B]: emg_score_triples of pos */
    uint64_t seed; uint64_t draw_counter;          /* draw_counter = epoch * batches_count + batch, both 0-based */
    double label_pos; double label_neg;            /* (n_pos + 1) / (n_pos + 2), 1 / (n_neg + 2)  (:2443-2454) */
    double weight_pos; double weight_neg;          /* #negative / #positive scores of the batch, (1 - rate) / rate  (:2491-2499) */
    double lr; double beta1; double beta2; double eps;   /* Keras defaults: 1e-3, 0.9, 0.999, 1e-7  (:2509) */
    double* state;                                 /* double [8], see above */
    void* workspace; int64_t workspace_bytes;
    int32_t* dbg_neg; float* dbg_scores;
} emg_calib_args;
int emg_calib_step(const emg_calib_args* args, void* stream);

/* Calibration WITH negatives (:2262-2287, :2421-2424): out[6] = {loss, dL/dw, dL/db, d2L/dw2, d2L/dwdb, d2L/db2} of the
 * objective over the n_pos + n_neg given scores at (w, b), for the host's Newton iteration (AmpliGraph: L-BFGS to
 * convergence).  The per-score terms and the reduction are emg_calib_step's (double, fixed order).  out: device double [6]. */
int emg_calib_moments(const float* scores_pos, int64_t n_pos, const float* scores_neg, int64_t n_neg, double w, double b,
                      double label_pos, double label_neg, double weight_pos, double weight_neg, double* out,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* _predict_proba (:2564-2570): out[i] = sigmoid(-(w scores[i] + b)), float [n] */
int emg_calib_proba(const float* scores, int64_t n, float w, float b, float* out, void* stream);

/* ---- embedding-space discovery (csrc/emg_neigh.hip; AmpliGraph 1.x find_nearest_neighbours / find_duplicates).  Rows are
 * embeddings as they are stored (ComplEx / HolE: the whole 2k row); no link function, no edge weight.  Two distances:
 *   EMG_METRIC_L2      sqrtf of the k-ordered chain acc = fmaf(d, d, acc), d = a_k - b_k: the bits of the negated
 *                      EMG_TRANSE_L2 entry of emg_eval_scores_dense(precision 0) for the same two rows;
 *   EMG_METRIC_COSINE  1 - dot, dot the k-ordered chain acc = fmaf(a_k, b_k, acc) over rows that emg_rows_normalize made
 *                      (the caller normalises; the join itself does not).
 * Distances are compared as unquantised f32. */
#define EMG_METRIC_L2 0
#define EMG_METRIC_COSINE 1

/* dst row = src row / sqrtf(chain sum of squares of the row, k ascending), element by element (correctly rounded division);
 * a row whose sum of squares is 0 becomes all zeros.  Columns [k_int, ld_dst) of dst are left as they are. */
int emg_rows_normalize(const float* src, int64_t n_rows, int64_t ld_src, int32_t k_int, float* dst, int64_t ld_dst, void* stream);

/* The radius join: every row of A [n_a, k_int] against every row of B [n_b, k_int].  self_offset >= 0: A row i IS B row
 * self_offset + i (A = B: 0) and that one pair is skipped — it is neither counted, nor a nearest row, nor written;
 * self_offset = -1: A is foreign to B, nothing is skipped.
 *   count[i]    int32: the B rows with d(i, j) <= radius (boundary included);
 *   nn_dist[i], nn_id[i]: the nearest other row, the lowest j among equally near ones; (+inf, -1) if there is none (NaN
 *               distances are no candidates);
 *   pairs       NULL, or room for pairs_capacity entries: every (i, j) with d <= radius as (i << 32 | j), in no particular
 *               order (the SET is deterministic).  pair_count uint64[2]: [0] the entries written, [1] != 0 if there were more
 *               than pairs_capacity — count and nn_* are complete all the same, nothing is written past the capacity, and a
 *               second call with a capacity of sum(count) gets them all.  pair_count may be NULL if pairs is.
 * Asynchronous on `stream`; no workspace.  n_a, n_b <= INT32_MAX. */
int emg_rows_within(int metric, const float* A, int64_t n_a, int64_t ld_a, const float* B, int64_t n_b, int64_t ld_b,
                    int32_t k_int, int64_t self_offset, float radius, int32_t* count, float* nn_dist, int32_t* nn_id,
                    uint64_t* pairs, int64_t pairs_capacity, uint64_t* pair_count, void* stream);

/* ---- clusters (csrc/emg_cluster.hip; AmpliGraph 1.x find_clusters with its default algorithm): an exact DBSCAN.  Rows, metrics
 * and distances are those above; distances are compared unquantised in f32 as d <= eps (boundary included), and both
 * distances are bit-symmetric in (i, j).  With N(i) the rows within eps of row i, i itself included:
 *   core rows    row i is core iff |N(i)| >= min_samples (scikit-learn's rule: the row itself counts);
 *   clusters     the connected components of the core rows under d <= eps, numbered 0, 1, ... in ascending order of their
 *                lowest core row index;
 *   border rows  a row that is not core but has a core row within eps takes the LOWEST label among its core neighbours'
 *                clusters;
 *   noise        every other row: -1.
 * This is what sklearn.cluster.DBSCAN(eps, min_samples).fit_predict returns (it expands clusters in index order and a border
 * row keeps the first label that reaches it), so the result is fully determined, border rows included.
 *   labels   int32 [n];  is_core uint8 [n] (1: core);  info int64 [2], device, 8-byte aligned: {clusters, noise rows}.
 *   ws       device, 16-byte aligned, at least emg_rows_dbscan_ws_bytes(n, min_samples) bytes (0: arguments out of range):
 *            16 + 28 n + 12 ceil(n / 1024) + 4 n min(max(min_samples - 2, 0), n - 1) bytes, each array rounded up to 16 — the
 *            count pass's outputs, parent / root / rank / list length per row, per-workgroup partial sums, and the border
 *            lists (a row that is not core has at most min_samples - 2 other rows within eps).  Contents need no
 *            initialisation; after the call its first int64 holds the longest parent chain the finish walked (a diagnostic).
 * Three passes on `stream`: emg_rows_within without pairs (counts), the same tile stream again (unions of core rows by
 * agent-scope compare-and-swap, border lists), and four small launches (roots, an exact scan, labels, info).  No host read,
 * no allocation.  n == 0 succeeds with info = {0, 0}.  EMG_EINVAL: unknown metric, n outside [0, INT32_MAX], k_int <= 0,
 * ld < k_int, eps NaN or negative, min_samples < 1, a workspace that is too small or misaligned (nothing is launched).
 * These symbols are additions: EMG_ABI_VERSION stays 9. */
size_t emg_rows_dbscan_ws_bytes(int64_t n, int32_t min_samples);
int emg_rows_dbscan(int metric, const float* X, int64_t n, int64_t ld, int32_t k_int, float eps, int32_t min_samples,
                    int32_t* labels, uint8_t* is_core, int64_t* info, void* ws, size_t ws_bytes, void* stream);

/* ---- k-means (csrc/emg_kmeans.hip; the estimator emgraph_amd.discovery.KMeans that find_clusters runs on the device).
 * Euclidean only: d(i, j) is the EMG_METRIC_L2 distance above between row i and centre j, formed by the same tile stream as
 * emg_rows_within (the same bits).  No sample weights.
 *   assignment  label[i] = the lowest j among the nearest centres, distances compared as unquantised f32.  A NaN distance is
 *               no candidate; a row without a candidate gets label -1, joins no mean and adds nothing to the inertia (the rule
 *               of emg_rows_within).
 *   update      centre[j] = (float)(sum of (double)x_i / (double)count_j) over the members of cluster j in ONE fixed order: the
 *               members in ascending row order (a stable counting sort of the rows by label), cut into chunks of 256; each
 *               chunk is added one member after the other starting from 0.0, then the chunk sums are added one after the other
 *               starting from 0.0.  No floating-point atomics: two runs give the same bits.  An EMPTY cluster KEEPS its centre
 *               (scikit-learn relocates it).
 *   inertia     the f64 sum of (double)d_i (double)d_i over the labelled rows, in a fixed order (a tree per 256 rows, then
 *               the blocks strided over 256 lanes and the same tree).
 *   stopping    after an update and the assignment against the new centres, the run stops when no label changed, or when
 *               sum_j |c_new - c_old|^2 (f64) <= tol_abs = tol * mean over columns of var(X) — the variance in f64, two-pass
 *               (means first, then squared deviations; both summed over chunks of 256 consecutive rows as the update sums a
 *               cluster), scikit-learn's _tolerance.  n_iter counts the updates done.  Every update is followed by an
 *               assignment, so the returned labels and inertia always belong to the returned centres, also after max_iter.
 *               A NaN anywhere in X makes tol_abs a NaN: the shift then never stops the run.
 * emg_rows_kmeans: ONE Lloyd run from the centres given, centres [n_clusters, k_int] (leading dimension ld_c) updated in place.
 *   labels   int32 [n];  info: device, 8-byte aligned, 32 bytes {double inertia, int64 n_iter, int64 converged, double tol_abs};
 *   max_iter = 0: assignment and inertia only (predict; tol_abs is reported as 0, the table's variance is not computed).
 *   ws       device, 16-byte aligned, at least emg_rows_kmeans_ws_bytes(n, n_clusters, k_int) bytes (0: arguments out of
 *            range): about 16 n + n n_clusters / 64 + 8 (n / 256 + n_clusters) k_int bytes.  Needs no initialisation.
 * Asynchronous on `stream`, no allocation and NO HOST READ: the launches of all max_iter iterations are enqueued at once, and
 * once the device-side "done" flag is set those of the remaining iterations exit at once.
 * emg_rows_kmeans_seed: k-means++ seeding (plain D^2 sampling; scikit-learn's greedy local trials are not mirrored).  Centre 0
 * is row first_row.  For c = 1 .. n_clusters - 1: m_i = the distance (the chain above, a NaN is no candidate) from row i to the
 * nearest centre chosen so far, updated with one n x 1 pass per pick; w_i = (double)m_i (double)m_i (0 where m_i is not
 * finite); S = the inclusive f64 prefix sum of w, formed as S_i = P_s + r_i: rows in segments of 256, r_i the running sum
 * inside segment s from 0.0, P_s the segment totals added one after the other from 0.0 (S is non-decreasing and S_n = the sum of
 * all totals).  The pick is the first i with S_i > u[c - 1] S_n (the last row if there is none); floor(u[c - 1] n) if S_n == 0.
 *   u        HOST pointer, n_clusters - 1 doubles in [0, 1) (read while the launches are enqueued);
 *   chosen   device int32 [n_clusters]: the rows picked; each pick is written to device memory and the next distance pass
 *            reads the centre from there — no host read.
 * EMG_EINVAL before anything is launched: n outside [1, INT32_MAX], n_clusters outside [1, n], k_int < 1, ld or ld_c < k_int,
 * max_iter < 0, tol negative / NaN / inf, first_row outside [0, n), u outside [0, 1), a null pointer, a workspace that is too
 * small or misaligned.  These symbols are additions: EMG_ABI_VERSION stays 9. */
size_t emg_rows_kmeans_ws_bytes(int64_t n, int64_t n_clusters, int32_t k_int);
int emg_rows_kmeans(const float* X, int64_t n, int64_t ld, int32_t k_int, float* centres, int64_t ld_c, int64_t n_clusters,
                    int32_t max_iter, double tol, int32_t* labels, void* info, void* ws, size_t ws_bytes, void* stream);
int emg_rows_kmeans_seed(const float* X, int64_t n, int64_t ld, int32_t k_int, int64_t n_clusters, int64_t first_row,
                         const double* u, float* centres, int64_t ld_c, int32_t* chosen, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMGRAPH_HIP_H */
