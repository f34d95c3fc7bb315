/*
 * dne_hip.h -- C ABI of libdne_hip.so, the MI355X (gfx950) ES/GA rollout-and-aggregate engine.
 *
 * Drop-in boundary for the hot path of uber-research/deep-neuroevolution's es_distributed/ CPU path.
 * The reference has no FFI on that path (its seams are Python call signatures); each entry
 * point below names the reference code it replaces (paths relative to the upstream repository root).
 * The reference-side binding a maintainer adds is the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions: every call returns 0 on success, <0 on error (dne_last_error gives the text); the caller
 * owns all host buffers, the engine owns all device memory; plain pointers and sizes only (no torch
 * types); a handle is bound to one HIP device, one host thread per handle; no callbacks.
 * "member" = one episode slot (one perturbed policy + one environment).  For ES, members 2i and 2i+1
 * are the antithetic pair of noise index i (theta + sigma*eps, theta - sigma*eps).
 */
#ifndef DNE_HIP_H
#define DNE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNE_KIND_ES 0 /* ESAtariPolicy  es_distributed/policies.py:305-429 */
#define DNE_KIND_GA 1 /* GAAtariPolicy  es_distributed/policies.py:433-513 */
#define DNE_KIND_GA_LARGE 2 /* LargeModel of the GPU tree (conv 32/64/64, fc 512): gpu_implementation/neuroevolution/models/dqn.py:39-47.
                               Deep-GA: genomes with per-seed powers (dne_ga_set_init_scale + dne_ga_eval_powers).  ES as the GPU tree's es.py runs it
                               over any of its models: dne_set_theta (base slot 0, never handed to GA parents or children) + dne_es_eval
                               (antithetic pairs, no reference batch) + dne_es_update; a shard travels with dne_records_pack / dne_allgather_results */
#define DNE_KIND_ES_VBN 3 /* ModelVirtualBN of the GPU tree in its own flat layout: gpu_implementation/neuroevolution/models/batchnorm.py:52-123
                             (tensors in creation order, models/base.py:35-44, 166-178).  The ES kind's network, evaluation and entry points
                             (virtual batch norm, antithetic pairs, dne_es_eval / dne_es_update); no conv / fc biases, no BN gamma: each
                             BatchNorm/b is the shift after normalisation.  P = 1003824 + 257 * n_actions */
#define DNE_KIND_MAZE 4 /* the GPU tree's hard maze (gym_tensorflow/maze/) under SimpleClassifier (models/simple.py:29-35: dense 11 -> 16 -> 16 -> 2,
                           498 parameters); n_actions = 2, the raw outputs are the action.  A whole episode (400 steps) runs inside one kernel
                           (csrc/maze.h): dne_maze_set_walls, then dne_set_members + dne_eval_members or dne_es_eval (pairs (2i, 2i+1) over base slot 0,
                           no reference pass; env_seed is accepted and ignored: the episode is deterministic).  returns = -distance to the goal after
                           step 400, 0 under a shorter tslimit; bc (record_bc): float (x, y) after every step, [members][bc_max_steps][2].
                           bc_final_only = 1 is refused by dne_create: dne_maze_final_state has every member's final (x, y).
                           The P-generic calls work unchanged (dne_es_update, dne_weighted_sum, the optimizer calls, dne_records_pack / _set,
                           dne_es_update_gathered); dne_ga_*, dne_ref_pass, dne_env_*, dne_novelty*, dne_act and dne_debug_plan refuse the kind. */
#define DNE_KIND_CARTPOLE 5 /* the GPU tree's gym configuration (configurations/es_gym_config.json): gym.CartPole-v1 under SimpleClassifier on 4 inputs
                           (dense 4 -> 16 -> 16 -> 2, 386 parameters); n_actions = 2, action = the first maximum of the two logits.  A whole episode
                           (at most 500 steps) runs inside one kernel (csrc/cartpole.h): dne_set_members + dne_eval_members or dne_es_eval (pairs
                           (2i, 2i+1) over base slot 0, no reference pass); env_seed[i] is member i's reset seed.  returns = signreturns = the
                           episode's length (reward 1 per step); a non-NULL bc and bc_final_only = 1 are refused: dne_cartpole_final_state has
                           every member's final state.  The P-generic calls work as on DNE_KIND_MAZE; every Atari-only, maze-only and GA-only
                           call, dne_debug_plan and dne_debug_plan_act refuse the kind. */
#define DNE_KIND_PENDULUM 6 /* es_distributed's MujocoPolicy (policies.py:122-217) on the torque-limited pendulum swing-up (csrc/pendulum.h, DESIGN.md
                           section 14): observations normalised by ob_mean / ob_std and clipped to +-5, two hidden layers of one width under tanh or
                           relu, a continuous or uniformly binned action, optional Gaussian action noise, optional observation statistics.  The
                           shape comes in through dne_config.reserved: [0] the hidden width (64, 128 or 256), [1] the action mode (0 continuous,
                           1 uniform bins), [2] the nonlinearity (0 tanh, 1 relu); n_actions carries the outputs (1 continuous, 2..16 bins).
                           P = dne_pendulum_num_params(hidden, n_actions); dne_num_params answers -1.  A whole episode (200 steps, never done early)
                           runs inside one kernel, one workgroup per member: dne_set_members + dne_eval_members or dne_es_eval as on
                           DNE_KIND_CARTPOLE, after dne_pendulum_set_ob_stat.  bc, record_bc and bc_final_only are refused.  The P-generic calls work
                           as on DNE_KIND_MAZE; every Atari-only, maze-only, cart-pole-only and GA-only call, dne_debug_plan and dne_debug_plan_act
                           refuse the kind. */
#define DNE_KIND_MJMAZE 7 /* MujocoPolicy as on DNE_KIND_PENDULUM, on the deceptive hard maze of DNE_KIND_MAZE (csrc/mjmaze.h): 11
                           observations, the action space Box(-0.5, 0.5, (2,)), 400 steps never done early, the reward 0 until step 400 and minus the
                           distance to the goal there; the behaviour characterisation is the final (x, y), which is what NS-ES / NSR-ES with this
                           policy need.  dne_config.reserved as on DNE_KIND_PENDULUM; n_actions carries the outputs: 2 continuous, 2 B for B = 2..8
                           uniform bins a dimension.  P = dne_mjmaze_num_params(hidden, n_actions); dne_num_params answers -1.  An evaluation
                           (dne_set_members + dne_eval_members, or dne_es_eval; env_seed may be NULL: there is no reset seed) comes after
                           dne_maze_set_walls and dne_mjmaze_set_ob_stat.  Accepted beside the dne_mjmaze_* and the P-generic calls:
                           dne_maze_set_walls, dne_maze_final_state, dne_maze_archive_append / _clear / _size / _get, dne_maze_novelty and
                           dne_maze_novelty_last_ms.  bc, record_bc and bc_final_only are refused, and so is every other Atari, GA, maze-GA,
                           pool-novelty, cart-pole, pendulum, plan and dne_stepenv_* call (the maze one step at a time is DNE_KIND_MAZE's). */
#define DNE_KIND_DENSE 8 /* a dense policy of any small shape on one of the four step environments (csrc/dense.h): the
                           model half of concurrent_worker.py:56-67 beside the dne_stepenv_* environments.  dne_config.reserved: [0] the
                           environment (DNE_KIND_MAZE, DNE_KIND_CARTPOLE, DNE_KIND_PENDULUM or DNE_ENV_ACROBOT: 11 / 4 / 3 / 6 inputs and the
                           action convention),
                           [1] hidden layers L = 0..3 (0: models/simple.py:23-27 LinearClassifier), [2] nonlinearity (0 tanh, 1 relu),
                           [3..5] the L hidden widths, each 1..64, unused entries 0.  n_actions carries the outputs: maze 2 (the raw outputs
                           are the action), cart-pole 2 (the first maximum; a tie or a NaN gives 0), pendulum 1 (the raw output is the torque,
                           observations are raw), acrobot 3 (the first maximum; a NaN never wins).  The flat vector is in creation order: per layer w [in][out] row-major, then b [out].
                           P = dne_dense_num_params(...); dne_num_params answers -1.  dne_set_members + dne_eval_members, or dne_es_eval, run
                           whole episodes (reset from env_seed, which the maze does not read; to the environment's own limit or tslimit) and
                           leave the step-at-a-time batch as it was; dne_dense_final_state has the final states.  dne_stepenv_* work on the
                           environment of reserved[0], and dne_stepenv_act / dne_stepenv_run put the policy behind them.  dne_maze_set_walls
                           is accepted when the environment is the maze.  The P-generic calls work as on DNE_KIND_MAZE.  bc, record_bc and
                           bc_final_only are refused, and so is every Atari, GA, maze-GA, novelty, plan, cart-pole-only, pendulum-only and
                           mjmaze call. */
#define DNE_ENV_ACROBOT 9 /* gym.Acrobot-v1 (csrc/acrobot.h): an ENVIRONMENT id, not an engine kind -- dne_create refuses it as
                           policy_kind.  It is valid as reserved[0] of DNE_KIND_DENSE with n_actions = 3, as the kind argument of
                           dne_stepenv_dims (6 observations, 1 action value, 4 state doubles, int32 actions) and of the dne_stepenv_*_host,
                           dne_dense_*_host and dne_dense_bc_host twins.  State theta1, theta2, omega1, omega2; actions 0 / 1 / 2 (torque -1 / 0 /
                           +1); reward -1 a step and 0 on the terminal one; at most 500 steps. */
#define DNE_OB_BYTES (84 * 84 * 4)
#define DNE_RAM_BYTES 128
#define DNE_BN_FLOATS 608

#define DNE_PROC_CENTERED_RANK 0      /* es.py:281-282 */
#define DNE_PROC_SIGN 1               /* es.py:283-284 */
#define DNE_PROC_CENTERED_SIGN_RANK 2 /* es.py:285-286 */

#define DNE_OPT_ADAM 0 /* optimizers.py:35-50 */
#define DNE_OPT_SGD 1  /* optimizers.py:23-32 */

typedef struct dne_handle dne_handle;

typedef struct {
    int32_t device_id;
    int32_t policy_kind;  /* DNE_KIND_* */
    int32_t n_actions;    /* env.action_space.n: 2..18 (18 for Frostbite).  The SynthAtari fixture defines 18 actions in ALE order; an
                             engine with fewer uses the first n_actions of them.  dne_create refuses any other width. */
    int32_t max_members;  /* episode slots evaluated concurrently (ES: 2 * pairs per call) */
    int32_t ref_count;    /* size of the virtual-batch-norm reference batch (es.py:160-162: 128); multiple of 8 */
    int32_t ref_chunk;    /* members per reference-pass chunk (bounds scratch memory); 0 = default */
    int32_t record_bc;    /* 1: keep behaviour characterisations (ES: RAM per step, GA: final RAM) */
    int32_t bc_max_steps; /* ES BC capacity in steps per member (<= timestep limit) */
    int32_t profile_events; /* 1: bracket hot kernels with HIP events (dne_get_profile) */
    int32_t bc_final_only;  /* ES with record_bc: keep only each member's final RAM ([members][128], what es_modified.py's
                               dumps use: bc_vec[-1], es_modified.py:176,197) instead of the whole trajectory */
    int32_t reserved[6];    /* DNE_KIND_PENDULUM, DNE_KIND_MJMAZE: [0] hidden width, [1] action mode, [2] nonlinearity; DNE_KIND_DENSE: the
                               environment, the layers, the nonlinearity and the widths (see there); otherwise 0 */
} dne_config;

typedef struct { /* filled by dne_get_profile; times from HIP events on the engine's stream */
    double eval_ms;       /* wall of the last dne_*_eval call (events) */
    double fc_ms;         /* sum over launches of the streaming fc+act kernel in the last eval */
    int64_t fc_launches;
    int64_t fc_group_steps; /* sum over launches of groups processed (ES: pairs, GA: members) */
    int64_t env_steps;    /* sum of episode lengths of the last eval */
    double conv_ms, env_ms, ref_ms; /* other stages of the last eval (0 if not profiled) */
    double reduce_ms;     /* last dne_weighted_sum / dne_es_update aggregate kernel */
    double materialize_ms;/* last dne_materialize kernel */
    /* the streaming kernel proper (k_fc), without the small-count tail path (k_fc_cols + k_out) */
    double fc_full_ms;
    double fc_full_launches;
    double fc_full_units; /* env-steps (member-steps actually taken) processed by those launches */
    double fc_full_kind;  /* which kernel those launches were: 6 = k_lfc_pair (LargeModel: an antithetic pair's theta and eps rows fetched once for both members), 5 = k_fc_ring (the workgroup's noise rows through an LDS ring), 4 = k_fc_sub (one wave per sub-slice chain), 3 = k_fc_duo (table-ordered units), 2 = k_fc2 (two pairs per work item), 1 = k_fc */
    double fc_full_union_ms; /* time during which at least one of those launches was running (windows run them concurrently) */
    double reserved[1];
} dne_profile;

/* ---- lifecycle ------------------------------------------------------------------------------------ */
int dne_create(const dne_config *cfg, dne_handle **out);
void dne_destroy(dne_handle *h);
const char *dne_last_error(dne_handle *h); /* h may be NULL: error of the last failed dne_create */
int dne_num_params(int policy_kind, int n_actions); /* Policy.num_params, policies.py:22 */
int dne_get_profile(dne_handle *h, dne_profile *out);
/* Debugging aid with no reference counterpart: every device buffer of the handle lies between two poisoned 4 KiB zones;
 * returns the number of damaged zones (0 = no kernel wrote outside its buffer), <0 on a HIP error.  Also run by
 * dne_destroy.  Environment knobs: DNE_REDZONE=0 (off), DNE_TRACE=1 (stage breadcrumbs on stderr), DNE_DEBUG_SYNC=1
 * (synchronise and check after every launch set of an evaluation, naming the lock-step that failed). */
int dne_check_redzones(dne_handle *h);

/* ---- SharedNoiseTable (es.py:51-67) as one device buffer --------------------------------------------- */
int dne_noise_upload(dne_handle *h, const float *host, size_t count);          /* es.py:57-60 */
/* the same in pieces, so the table can be uploaded while it is being sampled (es.py:59 draws 250M numbers): */
int dne_noise_alloc(dne_handle *h, size_t count);
int dne_noise_write(dne_handle *h, size_t offset, const float *host, size_t count);
int dne_noise_get(dne_handle *h, int64_t idx, int dim, float *out_host);        /* es.py:63-64 get(i, dim) */

/* ---- flat parameters (tf_util.py:224-246 SetFromFlat/GetFlat; policies.py:99-103) -------------------- */
/* Base slots are shared with the GA store: dne_ga_eval* keeps its parents (and, with DNE_GA_MATERIALIZE, its children) in slots above 0
 * of its own choosing.  A slot above 0 that the caller writes -- dne_set_theta, dne_ga_rebuild, dne_ga_rebuild_powers -- stays the caller's
 * until dne_ga_set_init_scale, which frees every slot but 0: the store never hands it out or overwrites it, and a parent it had cached
 * there is forgotten and rebuilt in another slot when next needed. */
int dne_set_theta(dne_handle *h, int slot, const float *theta, size_t n); /* slot 0 = the ES parent theta */
int dne_get_theta(dne_handle *h, int slot, float *out, size_t n);
int dne_set_ref_batch(dne_handle *h, const uint8_t *ref /*[ref_count][84][84][4]*/, int count); /* policies.py:332-335 */

/* A1 es.py:412-419: out[i][0] = theta + sigma*noise[idx_i:], out[i][1] = theta - sigma*noise[idx_i:]
 * written to an engine-owned device buffer; out_host (n*2*P floats) may be NULL */
int dne_materialize(dne_handle *h, const int64_t *noise_idx, int n, float sigma, float *out_host);

/* ---- batched environment (wrap_deepmind over the device-resident stepper; atari_wrappers.py:204-222) -
 * shape follows the reference GPU tree's native op ABI (gym_tensorflow/tf_env.cpp:115-318) */
int dne_env_reset(dne_handle *h, int n, const uint32_t *seeds);
int dne_env_step(dne_handle *h, int n, const int32_t *actions, float *reward, int32_t *done);
int dne_env_observation(dne_handle *h, int n, uint8_t *out /*[n][84][84][4]*/);
int dne_env_ram(dne_handle *h, int n, uint8_t *out /*[n][128]*/);
int dne_env_set_observation(dne_handle *h, int n, const uint8_t *obs /*[n][84][84][4]*/);
/* emulator state injection (ALE's cloneState/restoreState is the nearest reference notion; used by the renderer parity
 * tests): RAM before / after the last raw frame of n members; the observation becomes 4 copies of the warped max frame,
 * as after a FrameStack reset (atari_wrappers.py:171-176) */
int dne_env_set_ram(dne_handle *h, int n, const uint8_t *ram_prev /*[n][128]*/, const uint8_t *ram_cur /*[n][128]*/);

/* ---- policy forward on explicit members (policies.py:319-330,374-375 / 449-459,469-470) ---------------
 * member i uses theta_i = base[base_slot[i]] + scale[i] * noise[noise_off[i]:]   (ES: scale = +-sigma) */
int dne_set_members(dne_handle *h, int n, const int32_t *base_slot, const int64_t *noise_off, const float *scale);
int dne_ref_pass(dne_handle *h, int n);                                   /* policies.py:399 (ES only) */
int dne_get_bn(dne_handle *h, int n, float *out /*[n][608] scale,shift per layer*/);
/* the batch moments behind them: what batch_norm(decay=0) leaves in moving_mean / moving_variance (policies.py:322-328),
 * i.e. the moving_mean / moving_variance datasets of a snapshot (policies.py:49-57); [n][608] mean,variance per layer */
int dne_get_bn_moments(dne_handle *h, int n, float *out);
int dne_act(dne_handle *h, int n, int32_t *actions, float *logits /*[n][n_actions] or NULL*/);
int dne_debug_activations(dne_handle *h, int member, float *y1 /*7056*/, float *y2 /*3872*/, float *y3 /*256*/);
/* The current members as the kernels will read them, in the engine's order: base slot, noise offset and scale of each (member i uses
 * base[slot[i]] + scale[i] * noise[off[i]:], as under dne_set_members), and caller_index[i] = the caller's index of engine member i.
 * dne_ga_eval* may reorder its members (DNE_GA_SORT) and, with DNE_GA_MATERIALIZE, points them at written-out vectors with scale 0;
 * after dne_set_members and dne_es_eval caller_index is the identity.  Returns the number of current members and fills at most cap
 * entries of each array (any may be NULL).  Launches no kernel; every kind. */
int dne_debug_members(dne_handle *h, int cap, int32_t *slot, int64_t *off, float *scale, int32_t *caller_index);
/* LargeModel engines (DNE_KIND_GA_LARGE): raw outputs of conv1 [441*32], conv2 / conv3 [121*64] and the fc [512] of one member after
   dne_act -- kernel-level parity against the oracle's orc_forward_large_debug (models/dqn.py:39-47). */
int dne_debug_activations_large(dne_handle *h, int member, float *y1, float *y2, float *y3, float *y4);

/* ---- the lock-step planner without a device (csrc/plan.h) ------------------------------------------------
 * Which kernels an evaluation launches is decided on the host from the DNE_* knobs, a few facts about the member set and the active
 * count.  dne_debug_plan runs that decision for one burst: it needs no GPU and no handle (like dne_num_params). */
typedef struct { /* what the planner reads beyond the knobs */
    double dense_scale;           /* table length / the stretch of it the evaluation's noise slices cover (1 unless a rank draws from its own share) */
    int32_t kind;                 /* DNE_KIND_* (dne_debug_plan takes it from its own argument) */
    int32_t members_materialized; /* the members are plain vectors (GA children written out) */
    int32_t uniform_base;         /* every member perturbs the same base slot */
    int32_t antithetic_slot0;     /* base slot 0 everywhere, members (2i, 2i+1) = (offset, +s), (the same offset, -s) */
    int32_t pair_sigma_uniform;   /* ... with ONE s */
    int32_t n_streams;            /* window streams (the engine has 4) */
    int32_t has_y3s, has_theta_perm, has_scaled_table; /* the buffers of k_fc_sub, k_fc_ring and the ring's sigma-scaled table exist */
    int32_t reserved[3];
} dne_plan_facts;
enum { DNE_CONV_LARGE, DNE_CONV_FUSED /* k_conv12 */, DNE_CONV_TAIL4 /* k_conv12t */, DNE_CONV_SPLIT /* k_conv1 + k_conv2 */ };
enum { DNE_FC_LFC_COLS, DNE_FC_LFC, DNE_FC_SUB, DNE_FC_QUAD, DNE_FC_TAIL, DNE_FC_COLS, DNE_FC_RING, DNE_FC_DUO, DNE_FC_FC2, DNE_FC_FC,
       DNE_FC_LFC_PAIR /* k_lfc_pair: the LargeModel's streamed fc over antithetic pairs */ };
typedef struct { /* one window of a burst: groups [lo, lo + cnt) of the active list */
    int32_t lo, cnt;
    int32_t wide;                 /* more than DNE_FC_TAIL_MAX groups (LargeModel: members): a streaming fc */
    int32_t skip;                 /* DNE_DEBUG_SKIP */
    int32_t conv, s1, s2, act2;   /* DNE_CONV_*; workgroups per member of conv1 / conv2 (LargeModel: of conv2 / conv3); y2 left as relu(bn2(y2)) */
    int32_t fc;                   /* DNE_FC_* */
    int32_t sub_spw, sub_blocks;  /* k_fc_sub: sub-slices per wave, workgroups */
    int32_t solo, sweep, fat, ring_scaled; /* k_fc_duo / k_fc_ring: one unit per wave, common table timeline, DNE_DUO_FAT, the scaled table */
    int32_t tail, spec, head_fused, render_fused; /* fused tail; speculative tail; k_tail_step behind the fc; ... rendering too */
    int32_t render_bands, render_wg; /* k_env_render: workgroups per frame, threads per workgroup */
    int32_t chain;                /* DNE_FC_CHAIN_MIN: the fc waits for the previous window's */
    int32_t reserved[2];
} dne_window_plan;
/* The burst that starts with `total` active groups of `gsize` members on an engine of `kind` with `n_actions` actions, knobs read from the
 * environment exactly as dne_create reads them: writes one row per window (at most cap), *nsub = the number of windows; returns 0.
 * whole_eval != 0: writes no rows and returns dne_profile.fc_full_kind of an evaluation that STARTS at that width. */
int dne_debug_plan(int kind, int n_actions, const dne_plan_facts *facts, int total, int gsize, dne_window_plan *out, int cap, int *nsub,
                   int whole_eval);
/* What dne_act (and dne_env_step) of n members launches on such an engine: outside an evaluation the members are one window of single
 * members under no burst regime (csrc/plan.h: act_window).  Writes that one row (lo = 0, cnt = n); returns 0, or -1 for DNE_KIND_MAZE
 * and n < 1.  Of the facts only kind and members_materialized matter (dne_set_members clears the latter).  No GPU, no handle. */
int dne_debug_plan_act(int kind, int n_actions, const dne_plan_facts *facts, int n, dne_window_plan *out);
/* The reference batch as unique convolution operands (csrc/ref_index.h), as dne_set_ref_batch builds it.  ref: [count][84][84][4] u8.
 * idx1 [count][441]: id of each conv1 patch (8x8x4 bytes of the zero-padded 88x88 image) among the distinct ones; patches [cap1][256]:
 * those, k = (kh * 8 + kw) * 4 + c; idx2 [count][121]: id of each conv2 window among the distinct ones; windows [cap2][16]: those, as
 * sixteen conv1 patch ids in (kh, kw) order, -1 = SAME padding.  Any output may be null; *U1 / *U2 = the numbers of distinct rows.
 * Returns 1 when the reference pass would take the dedup route on such a batch, 0 for the dense one, -1 when a table does not fit.
 * No GPU, no handle. */
int dne_debug_ref_index(const uint8_t *ref, int count, int32_t *idx1, uint8_t *patches, int cap1, int32_t *idx2, int32_t *windows, int cap2,
                        int *U1, int *U2);
/* 1: the reference pass of this engine runs on the unique operands of the batch last set, 0: on the dense kernels (the knobs name
 * another route, or the batch has too many distinct rows); *U1 / *U2 (may be null) as above, 0 when the engine builds no index. */
int dne_ref_dedup_active(dne_handle *h, int *U1, int *U2);
/* the value of one knob (by its DNE_* name) after defaults, environment and clamping, as dne_create would see it; -1: no such knob */
int dne_debug_knob(int kind, int n_actions, const char *name);
/* k_out -- the policy head behind the streaming fc kernels -- on inputs the caller lays out: kind DNE_KIND_ES (bn rows [n_members][608]) or
 * DNE_KIND_GA, groups of gsize 1 or 2 members over one noise slice each, 1 .. 32 actions, the fc sums as the fc kernels leave them
 * ([member][4][256], or [member][32][256] with sub_sums), an LDS reservation of 0 .. 64 KB as DNE_OUT_LDS_KB makes it.  y3, actions and
 * logits (may be NULL) are read and written back.  A test hook: no handle, every buffer is uploaded for the call. */
int dne_debug_out_head(int kind, int gsize, int n_actions, int n_members, const int32_t *list /*[n_groups] or NULL*/, int n_groups,
                       const float *noise, size_t noise_count, const float *base /*[P]*/, const int64_t *off /*[n_members]*/,
                       const float *scale /*[n_members]*/, const int32_t *done /*[n_members] or NULL*/, const float *bn, const float *sums,
                       int sub_sums, int reserve_lds_kb, float *y3 /*[n_members][256]*/, int32_t *actions /*[n_members]*/, float *logits);

/* ---- A1-A7: whole-batch evaluation ------------------------------------------------------------------ */
/* es.py:411-426 for n pairs at once: returns_n2/signreturns_n2/lengths_n2 are [n][2] like Result (es.py:18-23).
 * Engines: DNE_KIND_ES, DNE_KIND_ES_VBN (reference pass first), DNE_KIND_GA_LARGE (theta = base slot 0, no reference pass) and DNE_KIND_MAZE (see there);
 * DNE_KIND_GA refuses (its kernels take one member per group).  DNE_KIND_GA_LARGE has no behaviour trajectories: bc = final RAM [2n][128].
 * env_seed[2n]: per-episode environment seed (noop count = 1 + seed % 30).  bc (may be NULL, needs record_bc):
 * [2n][bc_max_steps][128] RAM trajectories (policies.py:410,418) */
int dne_es_eval(dne_handle *h, const int64_t *noise_idx, int n, float sigma, int tslimit,
                const uint32_t *env_seed, float *returns_n2, float *signreturns_n2, int32_t *lengths_n2,
                uint8_t *bc);
/* generic: members set by dne_set_members, one episode each (eval episodes es.py:388-405 use scale 0) */
int dne_eval_members(dne_handle *h, int n, int tslimit, const uint32_t *env_seed, float *returns,
                     float *signreturns, int32_t *lengths, uint8_t *bc);
/* ga.py:251-271 for n children: chains in CSR form; theta = normc(noise[s0]) + sigma*sum noise[s_k].
 * bc (may be NULL): final RAM [n][128] (policies.py:510) */
int dne_ga_eval(dne_handle *h, const int32_t *chain_offsets /*n+1*/, const int64_t *seeds, int n, float sigma,
                int tslimit, const uint32_t *env_seed, float *returns, float *signreturns, int32_t *lengths,
                uint8_t *bc);
/* ga.py:151-158 / 256-264: rebuild one genome into base slot `slot` (and optionally copy it out); a slot above 0 becomes the caller's (see dne_set_theta) */
int dne_ga_rebuild(dne_handle *h, int slot, const int64_t *seeds, int nseeds, float sigma, float *out_host);

/* The gpu tree's genome form (gpu_implementation/neuroevolution/models/base.py:118-149, ga.py:161-166): seeds =
 * ((idx0,), (idx1, power1), ...), theta = noise[idx0] * scale_by + sum_k power_k * noise[idx_k]; scale_by = the
 * per-parameter initial scale (base.py:190-201).  powers[] runs parallel to seeds[]; the root's entry is ignored. */
int dne_ga_set_init_scale(dne_handle *h, const float *scale_by, size_t n);
int dne_ga_rebuild_powers(dne_handle *h, int slot, const int64_t *seeds, const float *powers, int nseeds, float *out_host);
int dne_ga_eval_powers(dne_handle *h, const int32_t *chain_offsets /*n+1*/, const int64_t *seeds, const float *powers, int n,
                       int tslimit, const uint32_t *env_seed, float *returns, float *signreturns, int32_t *lengths,
                       uint8_t *bc);

/* ---- A8-A10: on-device reduce ------------------------------------------------------------------------ */
/* es.py:70-85, stable ties; numpy's order: a NaN ranks above everything else (+inf included), NaNs among themselves by index */
int dne_centered_ranks(dne_handle *h, const float *x, int n, float *out);
/* es.py:291-296: g = (sum_i w[i] * noise[idx[i]:idx[i]+P]) / denom, kept on device; g_host may be NULL */
int dne_weighted_sum(dne_handle *h, const int64_t *idx, const float *w, int n, float denom, float *g_host);
/* es.py:298 + optimizers.py: theta(slot 0) <- theta + step(-g + l2coeff*theta) using the device g */
int dne_optimizer_step(dne_handle *h, int opt_kind, float l2coeff, double stepsize, double beta1_or_momentum,
                       double beta2, double epsilon, double *update_ratio);
int dne_optimizer_reset(dne_handle *h); /* zero m, v, t (a fresh Adam/SGD, optimizers.py:24-27,36-43) */
/* nses.py:95-117,283-284 keeps one optimizer per meta-population member: swap its state in and out
 * (Adam: m, v, t ; SGD: v in `v`, m ignored).  Pointers may be NULL to skip a field. */
int dne_optimizer_get_state(dne_handle *h, float *m, float *v, int32_t *t);
int dne_optimizer_set_state(dne_handle *h, const float *m, const float *v, int32_t t);   /* 0 <= t <= 2^31 - 2: the next step adds one */
/* es.py:281-298 in one call: process returns (proc_mode), aggregate, optimizer step */
int dne_es_update(dne_handle *h, const int64_t *idx, const float *returns_n2, const float *signreturns_n2,
                  int n, int proc_mode, int opt_kind, float l2coeff, double stepsize, double beta1_or_momentum,
                  double beta2, double epsilon, double *update_ratio);

/* ---- (e) the exchange step between GPUs: the master's Result collection es.py:226-277 for co-located GPU workers ----
 * A pair's wire record is 32 bytes, little-endian: int64 noise_idx, float ret[2], int32 len[2], float signret[2]
 * (the per-pair fields of Result, es.py:18-23).  Pair i of the N-pair population is evaluated by rank i % nranks.
 * dne_comm_unique_id (rank 0) + dne_comm_init (every rank, same 128 bytes) build an RCCL communicator over xGMI;
 * librccl.so.1 is opened on demand, single-GPU use never touches it. */
int dne_comm_unique_id(void *out128);
int dne_comm_init(dne_handle *h, int rank, int nranks, const void *unique_id128);
/* ncclCommInitRank blocks until every rank arrives: a caller that bounds it runs dne_comm_init on a second host thread and, on
 * time-out, calls dne_comm_abort from the first.  The late dne_comm_init then returns DNE_COMM_DROPPED (-2) WITHOUT touching the
 * handle (no error text: dne_last_error is not meaningful for that code); the handle must not be destroyed while it is in flight. */
#define DNE_COMM_DROPPED (-2)
/* what the communicator itself reports (ncclCommUserRank / ncclCommCount); without a communicator: rank 0 of 1, *is_rccl = 0.
 * The launcher side of gpu_implementation/neuroevolution/concurrent_worker.py:129-142 (one worker per visible device) asks
 * dne_device_count for the number of HIP devices this process can see. */
int dne_comm_info(dne_handle *h, int *rank, int *nranks, int *is_rccl);
int dne_device_count(int *count);
/* a second engine of the same process and device (another workload) takes part in the owner's communicator */
int dne_comm_share(dne_handle *h, dne_handle *owner);
/* leave RCCL for good (the ranks agreed on another carrier, or an initialisation hangs on another thread) */
int dne_comm_abort(dne_handle *h);
/* sum (op 0) / max (op 1) of n <= 64 doubles over all ranks, then a device synchronise; n = 0: barrier */
int dne_comm_allreduce(dne_handle *h, double *inout, int n, int op);
/* generic all-gather of `bytes` host bytes per rank (the GA's 32-byte child records: parent index, fresh seed, return,
 * length -- the per-child content of a GA Result, ga.py:266-271); recv holds nranks * bytes in rank order */
int dne_comm_allgather(dne_handle *h, const void *send, size_t bytes, void *recv);
/* all-gather of the records of the n_local pairs this rank evaluated in its last dne_es_eval (any kind dne_es_eval accepts), taken from the device
 * accumulators; the gathered set stays on the device in global pair order.  records_out: [n_global] records or NULL */
int dne_allgather_results(dne_handle *h, int n_local, int n_global, void *records_out);
/* test hook: un-shard a [nranks][ceil(n_global / nranks)] all-gather result (host copy) into global pair order on the device */
int dne_debug_unshard(dne_handle *h, const void *gathered, int n_global, int nranks, void *ordered_out);
/* other transports (the redis Result path, gloo in the CPU tests): this rank's shard of its last dne_es_eval out / the gathered set in */
int dne_records_pack(dne_handle *h, int n_local, void *records_out /*[n_local]*/);
int dne_records_set(dne_handle *h, const void *records /*[n_global], global pair order*/, int n_global);
/* es.py:281-298 on the gathered device-resident records (identical on every rank -> bit-identical theta) */
int dne_es_update_gathered(dne_handle *h, int proc_mode, int opt_kind, float l2coeff, double stepsize,
                           double beta1_or_momentum, double beta2, double epsilon, double *update_ratio);

/* ga.py:145: indices of the top-T returns, ordered by (-return, arrival index); a NaN return is the greatest */
int dne_ga_select(dne_handle *h, const float *returns, int m, int t, int32_t *out_idx);

/* ---- A13 nses.py:12-32: novelty of one behaviour characterisation against an archive -------------------
 * The archive (MasterClient.add_to_novelty_archive / get_archive, dist.py:93-98) is append-only, so it can live on the
 * device: dne_archive_append uploads one entry, and the two novelty calls score against the resident archive when their
 * `archive` argument is NULL.  A non-NULL archive replaces the resident one (one-shot form). */
int dne_archive_append(dne_handle *h, const uint8_t *bc /*[bc_len][dim]*/, int bc_len, int dim);
int dne_archive_clear(dne_handle *h);
int dne_archive_size(dne_handle *h);
int dne_novelty(dne_handle *h, const uint8_t *archive /*concatenated rows*/, const int32_t *archive_len,
                int narchive, const uint8_t *bc, int bc_len, int dim, int k, double *out);
/* nses.py:381-382 for a whole evaluated batch: novelty of each of the n members' RAM trajectories recorded by
 * the last dne_es_eval / dne_eval_members (record_bc engines; member i has lengths[i] rows of 128 bytes, which
 * never leave the device) against the archive */
int dne_novelty_batch(dne_handle *h, const uint8_t *archive, const int32_t *archive_len, int narchive, int n,
                      const int32_t *lengths, int k, double *out);
/* nses.py:22-32 for a batch, on the device: novelty of n trajectories against the resident archive.
 * bcs == NULL: the n members recorded by the last dne_es_eval / dne_eval_members (record_bc, full trajectories; dim 128,
 *              lengths[i] in [1, bc_max_steps]);
 * bcs != NULL: n host trajectories, rows concatenated, lengths[i] >= 1 rows of `dim` bytes each.
 * A tiled distance kernel (v_dot4_u32_u8 cross terms, exact int64 sums) writes the [n][narchive] distances to device
 * scratch and a selection kernel sums each member's k smallest in ascending order: only the n results cross PCIe.
 * dne_novelty (n = 1, host rows) and dne_novelty_batch (the recorded trajectories) are this call behind their own checks. */
int dne_novelty_knn(dne_handle *h, const uint8_t *bcs, const int32_t *lengths, int n, int dim, int k, double *out);

/* ---- pool novelty over final RAM states (GA-NS on Atari; csrc/ram_novelty.h) ------------------
 * A point is 128 bytes: the final RAM a record_bc GA engine (or a record_bc + bc_final_only ES engine) keeps per member.  Member m of the n
 * members is scored against the resident archive's A points (dne_archive_append: every entry of length 1 and width 128) at combined slots
 * 0 .. A - 1 followed by the n members at combined slots A .. A + n - 1, the combined slot A + m left out -- by index, not by value.
 * S = the exact integer sum of squared byte differences, d = orc_bc_distance of two one-row trajectories (sqrt((double)S), then
 * sqrt(a * a + 0.0)); the order is (S, combined slot); novelty = the first kk = min(k, A + n - 1) distances of that order added one by one
 * into a double, divided by kk; neighbours (or NULL) receives those kk combined slots per member, in that order.
 * bc == NULL reads the first n members of the last dne_ga_eval / dne_ga_eval_powers / dne_eval_members / dne_es_eval, in the caller's member
 * order, where the evaluation left them, and those n are the population; a host bc [n][128] takes any n >= 1 on any Atari engine.
 * k_ram_novelty_pool fuses distances and selection: no n x (A + n) buffer exists.  dne_ram_novelty_pool_host is the same header on the CPU
 * (no handle, no GPU; narch may be 0 and archive NULL then, any k >= 1).
 * dne_archive_append_members appends the points of the last evaluation's members members[0 .. count - 1], in that order, as entries of
 * length 1 and width 128, device to device (k_ram_archive_gather); indices may repeat and are checked before anything is launched.
 * dne_archive_get_points reads count entries of length 1 back, from entry `first`.  dne_ram_novelty_last_ms: the scoring kernel of the last
 * dne_ram_novelty_pool between two device events, in milliseconds (-1 before the first).
 * Refused by name, the archive, the recorded points and every other state left as they were: a whole-episode, step or dense engine kind; for
 * the NULL form and the gather an engine whose bc buffer is absent or holds full trajectories, a call before any evaluation, n (an index)
 * beyond the last evaluation's members; k < 1, k > DNE_RAM_NOVELTY_KMAX; n < 1; an empty pool (n = 1 and A = 0); an archive whose width is
 * not 128 or that holds an entry of length != 1 (the first such entry is named); A + n above INT_MAX, the kernel's slot field; a missing
 * buffer; for the gather and the read-back count < 1 or an index out of range; a gather into an archive of another width (in
 * dne_archive_append's words). */
#define DNE_RAM_NOVELTY_KMAX 32
#define DNE_RAM_NOVELTY_TILE 256      /* combined slots k_ram_novelty_pool stages at a time */
#define DNE_RAM_NOVELTY_MEMBERS 4     /* members of one workgroup's tile */
int dne_ram_novelty_pool(dne_handle *h, const uint8_t *bc /*[n][128], or NULL*/, int n, int k, double *out /*[n]*/,
                         int32_t *neighbours /*[n][min(k, A + n - 1)], or NULL*/);
int dne_ram_novelty_pool_host(const uint8_t *bc /*[n][128]*/, int n, const uint8_t *archive /*[narch][128], or NULL with narch 0*/, int narch,
                              int k, double *out /*[n]*/, int32_t *neighbours /*or NULL*/);
int dne_archive_append_members(dne_handle *h, const int32_t *members /*[count]*/, int count);
int dne_archive_get_points(dne_handle *h, int first, int count, uint8_t *out /*[count][128]*/);
double dne_ram_novelty_last_ms(dne_handle *h);

/* ---- the hard maze (DNE_KIND_MAZE; csrc/maze.h) ---------------------------------------------------------------
 * header8 = disable, steps, start x, start y, heading, goal x, goal y, 0 as the maze file gives them (`steps` and `heading` travel with the file
 * and are not read: tf_maze.cpp ends an episode after 400 steps and reset() starts at heading 0); lines [n][4] = wall segments ax, ay, bx, by.
 * n outside 1..64 is refused.  An evaluation before dne_maze_set_walls is an error. */
int dne_maze_set_walls(dne_handle *h, const float *header8, const float *lines, int n);
/* MazeFinalState (tf_maze.cpp:154-200): the navigators' final (x, y) of the last evaluation's first n members -- the behaviour characterisation of NS-ES on the maze */
int dne_maze_final_state(dne_handle *h, int n, float *xy /*[n][2]*/);
/* The same source on the CPU: n thetas, one episode each.  Needs no handle and no GPU (like dne_debug_plan; dne_last_error(NULL) has the text of a
 * failure).  trace: [n][tslimit][16] or NULL; row t = the observation after step t (11 floats: what the policy sees next), then x, y, heading, speed,
 * ang_vel.  Rows past an episode's length (min(tslimit, 400)) are not written. */
int dne_maze_rollout_host(const float *theta /*[n][498]*/, int n, const float *header8, const float *lines, int n_walls, int tslimit,
                          float *returns, int32_t *lengths, float *xy /*[n][2]*/, float *trace);
/* the device twin of that trace for one of the current members (dne_set_members / dne_es_eval): the kernel once more, every step written out;
 * trace [min(tslimit, 400)][16].  The last evaluation's results stay as they are. */
int dne_maze_debug_trace(dne_handle *h, int member, int tslimit, float *trace);
/* CPU test hooks, no handle: the environment alone under n open-loop action sequences (actions [n][T][2]; rows [n][T][18] = obs[11], x, y, heading,
 * speed, ang_vel, collisions, reward after each step; obs0 [n][11] or NULL = the observation after reset), and the forward pass alone for n
 * (theta, observation) pairs (h1, h2 [n][16] after their relus, out [n][2]) */
int dne_maze_actions_host(const float *actions, int n, int T, const float *header8, const float *lines, int n_walls, float *rows, float *obs0);
int dne_maze_forward_host(const float *theta, const float *obs, int n, float *h1, float *h2, float *out);
/* The header's trigonometry outside an episode, for n inputs travelling as doubles; out [n][2].  fn 0: sincos_d(x) -> (sin, cos); 1: atan_d(x) ->
 * (atan, 0); 2: (float)x degrees -> to_rad_f -> sincos_f -> (sin, cos); 3: (float)x = ty / tx -> the goal's angle in degrees exactly as the radar
 * forms it -> (the tx > 0 value, the tx < 0 value).  dne_maze_math_host runs on the CPU (no handle), dne_maze_debug_math one thread per input on
 * the device; every kind but DNE_KIND_MAZE refuses the device call. */
int dne_maze_math_host(int fn, const double *x, int n, double *out);
int dne_maze_debug_math(dne_handle *h, int fn, const double *x, int n, double *out);

/* ---- gym.CartPole-v1 (DNE_KIND_CARTPOLE; csrc/cartpole.h) ---------------------------------
 * The state is four doubles: x, x_dot, theta, theta_dot.
 * dne_cartpole_final_state: the final states of the last evaluation's first n members (1 <= n <= the members that evaluation ran).
 * dne_cartpole_debug_trace: the kernel once more for ONE of the current members (dne_set_members / dne_es_eval), every step written out:
 * trace [min(tslimit, 500)][8] = the observation after the step (four float32 values as doubles), then the state; *steps = the episode's
 * length, rows past it are not written.  init4 != NULL is the initial state; NULL resets from the environment seed that member had in the
 * last evaluation (0 before any).  The accumulators of the last evaluation are left alone.  Every other kind refuses both calls.
 * The _host calls are the same header on the CPU (no handle, no GPU):
 *   dne_cartpole_reset_host    the reset state of one seed;
 *   dne_cartpole_rollout_host  one episode for each of n thetas [n][386] under seeds [n] (init4 [n][4] or NULL as above) -> returns, lengths,
 *                              final states [n][4], trace [n][tslimit][8] or NULL;
 *   dne_cartpole_actions_host  the environment alone: n sequences of T actions (0 / 1) from init4 [n][4] -> rows [n][T][5] = the state
 *                              after the step, then done (1 / 0); stepping goes on past done;
 *   dne_cartpole_forward_host  the policy alone: thetas [n][386] on observations [n][4] -> h1 [n][16], h2 [n][16], out [n][2]. */
int dne_cartpole_final_state(dne_handle *h, int n, double *state /*[n][4]*/);
int dne_cartpole_debug_trace(dne_handle *h, int member, int tslimit, const double *init4 /*[4] or NULL*/, double *trace, int32_t *steps);
int dne_cartpole_reset_host(uint32_t seed, double *out4);
int dne_cartpole_rollout_host(const float *theta, int n, const uint32_t *seeds, const double *init4, int tslimit, float *returns,
                              int32_t *lengths, double *state, double *trace);
int dne_cartpole_actions_host(const int32_t *actions, int n, int T, const double *init4, double *rows);
int dne_cartpole_forward_host(const float *theta, const float *obs, int n, float *h1, float *h2, float *out);

/* ---- MujocoPolicy on the pendulum (DNE_KIND_PENDULUM; csrc/pendulum.h) -------------------
 * dne_pendulum_num_params: P = 5 H + H^2 + H O + O, or -1 for a width or an output count the header does not build.
 * dne_pendulum_set_ob_stat: ob_mean [3] and ob_std [3] of the normalisation; NaN before the first call, and an evaluation is then refused.
 * dne_pendulum_set_rollout_options: for the NEXT evaluation only, which must run exactly n members: ac_off [n] (or NULL: no action noise) --
 *   member i adds fl(ac_noise_std * table[ac_off[i] + t]) to its action at step t, an offset < 0 means none; ac_off[i] + 200 must lie
 *   inside the noise table -- and stat_flag [n] (or NULL: no statistics) -- a flagged member accumulates the observations it acted on.
 * dne_pendulum_ob_stats: of the last evaluation's first n members: sum [n][3], sumsq [n][3] (doubles, in step order), count [n] (= the
 *   length; all zero for an unflagged member).  dne_pendulum_final_state: state [n][2] = (theta, theta_dot).
 * dne_pendulum_debug_trace: the kernel once more for ONE of the current members, without noise or statistics, every step written out:
 *   trace [min(tslimit, 200)][8] doubles = the three observations acted on, the net's action, the action applied (before the clip), the
 *   reward, theta and theta_dot after the step; init2 = an explicit (theta, theta_dot) instead of the reset.
 * dne_pendulum_debug_math: value by value on the device; fn 0 tanh_f((float)x), 1 norm_angle(x), 2 the normalise-and-clip of (float)x under
 *   mean a and deviation b.
 * The CPU twins need no handle and no GPU (errors through dne_last_error(NULL)):
 *   dne_pendulum_reset_host    (theta, theta_dot) of one seed;
 *   dne_pendulum_rollout_host  one episode for each of n thetas [n][P]: every input the kernel has (table / ac_off both or neither), every
 *                              output it writes, trace [n][tslimit][8] or NULL;
 *   dne_pendulum_actions_host  the environment alone: n sequences of T float actions from init2 [n][2] -> rows [n][T][3] = theta, theta_dot
 *                              after the step, the reward;
 *   dne_pendulum_forward_host  the policy alone on raw observations [n][3] -> x [n][3], h1 [n][H], h2 [n][H], out [n][O], action [n];
 *   dne_pendulum_math_host     dne_pendulum_debug_math on the CPU. */
int dne_pendulum_num_params(int hidden, int n_out);
int dne_pendulum_set_ob_stat(dne_handle *h, const float *mean /*[3]*/, const float *std /*[3]*/);
int dne_pendulum_set_rollout_options(dne_handle *h, int n, float ac_noise_std, const int64_t *ac_off /*[n] or NULL*/, const uint8_t *stat_flag /*[n] or NULL*/);
int dne_pendulum_ob_stats(dne_handle *h, int n, double *sum /*[n][3]*/, double *sumsq /*[n][3]*/, int32_t *count /*[n]*/);
int dne_pendulum_final_state(dne_handle *h, int n, double *state /*[n][2]*/);
int dne_pendulum_debug_trace(dne_handle *h, int member, int tslimit, const double *init2 /*[2] or NULL*/, double *trace, int32_t *steps);
int dne_pendulum_debug_math(dne_handle *h, int fn, const double *x, int n, float a, float b, double *out);
int dne_pendulum_reset_host(uint32_t seed, double *out2);
int dne_pendulum_rollout_host(const float *theta, int n, int hidden, int n_out, int ac_mode, int nonlin, const float *mean, const float *std,
                              const uint32_t *seeds, const double *init2, int tslimit, float ac_noise_std, const float *table, size_t table_len,
                              const int64_t *ac_off, const uint8_t *stat_flag, float *returns, float *signreturns, int32_t *lengths,
                              double *state, double *ob_sum, double *ob_sumsq, int32_t *ob_count, double *trace);
int dne_pendulum_actions_host(const float *actions, int n, int T, const double *init2, double *rows);
int dne_pendulum_forward_host(const float *theta, const float *obs, int n, int hidden, int n_out, int ac_mode, int nonlin, const float *mean,
                              const float *std, float *x, float *h1, float *h2, float *out, float *action);
int dne_pendulum_math_host(int fn, const double *x, int n, float a, float b, double *out);

/* ---- MujocoPolicy on the hard maze (DNE_KIND_MJMAZE; csrc/mjmaze.h) ----------------------
 * Each call is the sibling of its dne_pendulum_* namesake, on 11 observations and 2 action dimensions.
 * dne_mjmaze_num_params: P = 13 H + H^2 + H O + O, or -1 for a width or an output count the header does not build (O even, 2..16).
 * dne_mjmaze_set_ob_stat: ob_mean [11] and ob_std [11]; NaN before the first call, and an evaluation is then refused.
 * dne_mjmaze_set_rollout_options: for the NEXT evaluation only, which must run exactly n members: ac_off [n] (or NULL) -- where each member's
 *   800 action-noise values start in the noise table (step t, dimension i reads ac_off + 2 t + i), < 0 for none; ac_off + 800 must lie inside
 *   the table, checked here and again at the launch -- and stat_flag [n] (or NULL).
 * dne_mjmaze_ob_stats: sum [n][11], sumsq [n][11] (doubles, in step order), count [n] of the last evaluation's first n members.
 * dne_mjmaze_debug_trace: the kernel once more for ONE current member, without noise or statistics: trace [min(tslimit, 400)][20] floats = the
 *   11 observations acted on, the net's 2 actions, the 2 applied, then x, y, heading, speed, ang_vel after the step; *steps = the rows.
 * No handle, no GPU: dne_mjmaze_rollout_host (every input and output of the kernel; trace [n][tslimit][20] or NULL) and
 *   dne_mjmaze_forward_host (raw observations [n][11] -> x [n][11], h1 [n][H], h2 [n][H], out [n][O], action [n][2]). */
int dne_mjmaze_num_params(int hidden, int n_out);
int dne_mjmaze_set_ob_stat(dne_handle *h, const float *mean /*[11]*/, const float *std /*[11]*/);
int dne_mjmaze_set_rollout_options(dne_handle *h, int n, float ac_noise_std, const int64_t *ac_off /*[n] or NULL*/, const uint8_t *stat_flag /*[n] or NULL*/);
int dne_mjmaze_ob_stats(dne_handle *h, int n, double *sum /*[n][11]*/, double *sumsq /*[n][11]*/, int32_t *count /*[n]*/);
int dne_mjmaze_debug_trace(dne_handle *h, int member, int tslimit, float *trace, int32_t *steps);
int dne_mjmaze_rollout_host(const float *theta, int n, int hidden, int n_out, int ac_mode, int nonlin, const float *mean, const float *std,
                            const float *header8, const float *lines, int n_walls, int tslimit, float ac_noise_std, const float *table,
                            size_t table_len, const int64_t *ac_off, const uint8_t *stat_flag, float *returns, float *signreturns, int32_t *lengths,
                            float *xy, double *ob_sum, double *ob_sumsq, int32_t *ob_count, float *trace);
int dne_mjmaze_forward_host(const float *theta, const float *obs, int n, int hidden, int n_out, int ac_mode, int nonlin, const float *mean,
                            const float *std, float *x, float *h1, float *h2, float *out, float *action);

/* ---- the maze, the cart-pole and the pendulum one step at a time (csrc/step_env.h) ------------------------------
 * The seam of gym_tensorflow/tf_env.py (reset / step / observation / final_state apart from the model) on the three whole-episode kinds: a
 * batch of max_members environments per handle that persists between calls and moves one step per call under actions the CALLER supplies, so
 * any policy can drive them.  It is allocated by the first call that needs it and is apart from evaluations: dne_eval_members, dne_es_eval
 * and dne_maze_ga_eval leave it as it was, and no call here touches members, accumulators or final states.
 * One environment is a state of S doubles, the steps taken, its step limit, done and its last observation:
 *   DNE_KIND_MAZE      S 7: x, y, heading, speed, ang_vel, collide, collisions (maze.h's floats and ints, widened exactly); 11 observations;
 *                      action float[2]; own limit 400
 *   DNE_KIND_CARTPOLE  S 4: x, x_dot, theta, theta_dot; 4 observations; action int32 in {0, 1}; own limit 500
 *   DNE_KIND_PENDULUM  S 2: theta, theta_dot; 3 observations (raw: normalising is the policy's business); action float[1]; own limit 200
 *   DNE_ENV_ACROBOT    S 4: theta1, theta2, omega1, omega2; 6 observations (cos, sin of each angle, the velocities); action int32 in {0, 1, 2};
 *                      own limit 500.  No engine kind of its own: a DNE_KIND_DENSE engine created on it steps it
 * dne_stepenv_dims: the four widths of a kind, no handle needed (-1 for every other kind; a NULL output is skipped).
 * indices [n] name the environments of a call, distinct, each in 0 .. max_members - 1; NULL means 0 .. n - 1.  Every per-call array is [n] in
 * the order of that list, and environments the list does not name keep every bit.
 * dne_stepenv_reset: the maze restarts from its header (seeds is not read and may be NULL), the other two from reset_state(seeds[i]); steps 0,
 *   done 0, limit = min(max_steps, own limit), max_steps <= 0 meaning the own limit.
 * dne_stepenv_step_f32 (maze, pendulum) / _i32 (cart-pole, acrobot): one step each.  Maze: reward = -(distance to the goal) on the step that makes
 *   steps == 400 and 0 otherwise, done when steps == limit.  Cart-pole: reward 1 per step taken, done when a threshold is crossed (strictly)
 *   or steps == limit.  Pendulum: the step's float32 reward, done when steps == limit.  Acrobot: reward -1 per step and 0 on the terminal one, done when the
 *   free end rises above the line (strictly) or steps == limit.  A done environment stepped again: reward 0, done 1,
 *   state, steps and observation unchanged.
 * dne_stepenv_observation: what a whole-episode kernel's policy would see next.  dne_stepenv_get_state: state [n][S], steps, done (a NULL
 *   output is skipped).  dne_stepenv_set_state: the analogue of dne_env_set_ram -- states no reset gives (rounded to the maze's own types),
 *   steps[i] in 0 .. limit - 1; the observation is recomputed and done cleared.
 * dne_stepenv_last_ms: the last step kernel between two device events, in milliseconds (-1 before the first, or on another kind).
 * All calls are ordered on the engine's stream and return when their outputs are on the host.  Refused by name, the batch left as it was: a
 * handle of another kind; _i32 on the maze or the pendulum, _f32 on the cart-pole; n outside 1 .. max_members; an index out of range or named
 * twice; stepping, observing or reading an environment that was never reset; the maze before dne_maze_set_walls; a cart-pole action outside
 * {0, 1} or an acrobot action outside {0, 1, 2} (checked on the host before the launch); NULL seeds on the cart-pole or the pendulum.  dne_env_* keep refusing the three kinds.
 * The CPU twins need no handle and no GPU (errors through dne_last_error(NULL)); they work on the caller's arrays of n environments (header8 /
 * lines / n_walls for the maze, else NULL / 0) and run the same header: dne_stepenv_reset_host, dne_stepenv_step_host (actions: float [n][2],
 * int32 [n] or float [n] by kind), dne_stepenv_observe_host (the observations of given states). */
int dne_stepenv_dims(int kind, int *obs, int *act, int *state, int *act_is_int);
int dne_stepenv_reset(dne_handle *h, int n, const int32_t *indices /*[n] or NULL*/, const uint32_t *seeds /*[n]; maze: may be NULL*/, int max_steps);
int dne_stepenv_step_f32(dne_handle *h, int n, const int32_t *indices, const float *actions /*[n][act]*/, float *reward, uint8_t *done);
int dne_stepenv_step_i32(dne_handle *h, int n, const int32_t *indices, const int32_t *actions /*[n]*/, float *reward, uint8_t *done);
int dne_stepenv_observation(dne_handle *h, int n, const int32_t *indices, float *obs /*[n][obs]*/);
int dne_stepenv_get_state(dne_handle *h, int n, const int32_t *indices, double *state /*[n][S]*/, int32_t *steps, uint8_t *done);
int dne_stepenv_set_state(dne_handle *h, int n, const int32_t *indices, const double *state, const int32_t *steps, int max_steps);
double dne_stepenv_last_ms(dne_handle *h);
int dne_stepenv_reset_host(int kind, int n, const uint32_t *seeds, const float *header8, const float *lines, int n_walls, int max_steps,
                           double *state, int32_t *steps, int32_t *limit, uint8_t *done, float *obs);
int dne_stepenv_step_host(int kind, int n, const void *actions, const float *header8, const float *lines, int n_walls, double *state,
                          int32_t *steps, const int32_t *limit, uint8_t *done, float *reward, float *obs);
int dne_stepenv_observe_host(int kind, int n, const double *state, const float *header8, const float *lines, int n_walls, float *obs);
/* the acrobot alone (csrc/acrobot.h): n sequences of T actions (0 / 1 / 2) from init4 [n][4] -> rows [n][T][5] = the state after the step, then
 * terminal (1 / 0); stepping goes on past it.  No handle, no GPU. */
int dne_acrobot_actions_host(const int32_t *actions, int n, int T, const double *init4, double *rows);

/* ---- dense policies of any small shape on the step environments (DNE_KIND_DENSE; csrc/dense.h) ----
 * dne_dense_num_params: P of a shape (widths: n_hidden entries), or -1 for a shape that is not built.
 * dne_dense_env_kind: the environment of a DNE_KIND_DENSE engine (its reserved[0]); the kind itself on every other engine.
 * dne_dense_final_state: the final states [n][S] of the last evaluation, in the record format of the dne_stepenv_* calls.
 * dne_stepenv_act: the forward pass of member members[i] (0 .. members set - 1, repeats allowed; members == NULL: members[i] = indices[i])
 * on the current observation of environment indices[i]: out [n][outputs] and the actions as dne_stepenv_step_* take them (maze float [n][2],
 * cart-pole int32 [n], pendulum float [n]), each unless NULL.  Nothing on the device changes.
 * dne_stepenv_run: max_steps >= 1 rounds of act -> step in ONE launch, from the batch's current state, which is written back; an
 * environment stops when it is done (and one that was done keeps every bit).  reward_sum [n]: the float64 sum of the rewards of this call
 * in step order, cast once; steps_taken [n]: the steps this call took; done [n]; each unless NULL.
 * Both are refused by name, with nothing changed: on another kind, when no members are set or a member index is out of range, for
 * max_steps < 1 (dne_stepenv_run), and for everything dne_stepenv_step_* refuses.  dne_stepenv_last_ms covers the run kernel too.
 * dne_dense_forward_host / dne_dense_rollout_host: the same header on the CPU, no handle, no GPU, errors through dne_last_error(NULL).
 * theta [n][P].  layers (may be NULL): per row the hidden layers' activations behind their nonlinearity, concatenated; out [n][outputs];
 * action (may be NULL) as dne_stepenv_act's.  The rollout resets from seeds (the maze reads none) or starts from init_state [n][S], runs to the
 * environment's own limit or tslimit and leaves returns, signreturns (may be NULL), lengths and the final state [n][S]. */
#define DNE_DENSE_TANH 0
#define DNE_DENSE_RELU 1
int dne_dense_num_params(int env_kind, int n_hidden, const int32_t *widths, int n_out);
int dne_dense_env_kind(dne_handle *h);
int dne_dense_final_state(dne_handle *h, int n, double *state /*[n][S]*/);
int dne_stepenv_act(dne_handle *h, int n, const int32_t *indices, const int32_t *members, float *out /*[n][O] or NULL*/, void *actions /*[n][act] or NULL*/);
int dne_stepenv_run(dne_handle *h, int n, const int32_t *indices, const int32_t *members, int max_steps, float *reward_sum, int32_t *steps_taken,
                    uint8_t *done);
int dne_dense_forward_host(const float *theta, const float *obs, int n, int env_kind, int n_hidden, const int32_t *widths, int nonlin, int n_out,
                           float *layers, float *out, void *action);
int dne_dense_rollout_host(const float *theta, int n, int env_kind, int n_hidden, const int32_t *widths, int nonlin, int n_out, const uint32_t *seeds,
                           const double *init_state, const float *header8, const float *lines, int n_walls, int tslimit, float *returns,
                           float *signreturns, int32_t *lengths, double *state);

/* ---- Deep-GA on a dense policy (DNE_KIND_DENSE; csrc/dense_ga.h) -----------------------------
 * The Deep-GA surface of the hard maze (dne_maze_ga_*, below) for a dense policy of any shape: P is the handle's, the arithmetic is
 * csrc/maze_ga.h's.  A bank of T <= max_members parents lives on the device, apart from the base slots; a member is (parent, idx, power):
 *   root   parent == -1, idx >= 0      theta_p = fl(noise[idx + p] * scale_by[p])                (power is not read)
 *   child  0 <= parent < T, idx >= 0   theta_p = bank[parent][p] + fl(power * noise[idx + p])     (never fused)
 *   kept   0 <= parent < T, idx < 0    bank[parent] bit for bit: dne_dense_ga_promote only
 * dne_dense_ga_set_init_scale takes scale_by [P] (policies.dense_scale_by of the shape) and allocates the bank: 3 * max_members slots (two
 * halves of a double buffer and one scratch slot per member) and the GA's own descriptor arrays.  dne_dense_ga_build fills the bank with T
 * parents from their genomes (chain_offsets [T + 1] into seeds / powers, from 0).  dne_dense_ga_eval runs one episode per root / child member
 * in one k_dense_run launch; member i is reset from env_seed[i] on the cart-pole and the pendulum (required there; the maze reads none, NULL
 * is fine).  dne_dense_final_state, dne_get_profile and dne_stepenv_last_ms follow it as they follow dne_eval_members.  dne_dense_ga_promote
 * makes the theta of descriptor j the new parent j, for all T_new at once and from the bank as it was: a kept parent may move to another
 * index and two descriptors may name one source.  dne_dense_ga_parents returns T (-1 on another kind), dne_dense_ga_get_parent copies one
 * parent [P] out.  All are ordered on the engine's stream.
 * Refused by name, with the bank left bit for bit as it was: another kind, no init scale, no noise table, (evaluation) no maze loaded on
 * the maze and a NULL env_seed elsewhere, n or T outside 1 .. max_members, a parent >= T or any parent on an empty bank, the kept form in
 * an evaluation, idx + P past the table, an empty chain or chain_offsets[0] != 0, a missing buffer, tslimit <= 0.
 * None of these reads or writes the base slots, the members of dne_set_members or the step-at-a-time batch.
 * dne_dense_ga_theta_host / dne_dense_ga_members_host are the same header on the CPU (no handle, no GPU; P in 1 .. 9218): the theta of one
 * genome, and of n descriptors -- the kept form included -- against a host bank [T][P] (NULL when T == 0); errors through dne_last_error(NULL). */
int dne_dense_ga_set_init_scale(dne_handle *h, const float *scale_by, size_t n /*P*/);
int dne_dense_ga_build(dne_handle *h, int T, const int32_t *chain_offsets /*T+1*/, const int64_t *seeds, const float *powers);
int dne_dense_ga_eval(dne_handle *h, int n, const int32_t *parent, const int64_t *idx, const float *power, const uint32_t *env_seed /*n or NULL*/,
                      int tslimit, float *returns, float *signreturns /*or NULL*/, int32_t *lengths);
int dne_dense_ga_promote(dne_handle *h, int T_new, const int32_t *parent, const int64_t *idx, const float *power);
int dne_dense_ga_parents(dne_handle *h);
int dne_dense_ga_get_parent(dne_handle *h, int j, float *out /*P*/);
int dne_dense_ga_theta_host(const float *noise, size_t count, const float *scale_by, int P, const int64_t *seeds, const float *powers, int nseeds,
                            float *out /*P*/);
int dne_dense_ga_members_host(const float *noise, size_t count, const float *scale_by, int P, const float *bank /*[T][P]*/, int T,
                              const int32_t *parent, const int64_t *idx, const float *power, int n, float *out /*[n][P]*/);

/* ---- Deep-GA on MujocoPolicy (DNE_KIND_PENDULUM and DNE_KIND_MJMAZE; csrc/mujoco_ga.h) ---------
 * es_distributed/ga.py's genome for this policy: the root is the policy REINITIALISED on a noise slice (ga.py:256-260) -- every weight column
 * of l0/w, l1/w and out/w scaled to norm 1 (std 1.0 for all three, `out` included), every bias +0 --, then per further seed
 * theta += fl(sigma * noise[seed ..]).  The scale is one value a column, sc = 1.0f / sqrtf(sum_k fl(x * x)), the sum in numpy's order for
 * np.square(x).sum(axis=0) on the [K][C] view: sequential in k for C >= 2, numpy's pairwise order for the one-column out/w [H][1].
 * A bank of T <= T_max parents lives on the device, apart from the base slots; a member is (parent, idx, power):
 *   root   parent == -1, idx >= 0      the root rule above                                        (power is not read)
 *   child  0 <= parent < T, idx >= 0   theta_p = bank[parent][p] + fl(power * noise[idx + p])     (never fused)
 *   kept   0 <= parent < T, idx < 0    bank[parent] bit for bit: dne_mujoco_ga_promote only
 * dne_mujoco_ga_reserve allocates the bank (2 * T_max slots, a double buffer; empty) and the GA's own descriptor arrays; called again it
 * starts over with an empty bank.  The scratch slots of an evaluation's roots are allocated by the first evaluation that has a root.
 * dne_mujoco_ga_build fills the bank with T parents from their genomes (chain_offsets [T + 1] into seeds / powers, from 0; powers[0] of a
 * chain is not read).  dne_mujoco_ga_eval runs one episode per root / child member in one k_pendulum_rollout / k_mjmaze_rollout launch;
 * member i is reset from env_seed[i] on the pendulum (required there; the maze reads none, NULL is fine).  It honours
 * dne_*_set_rollout_options and needs dne_*_set_ob_stat as dne_eval_members does; dne_*_ob_stats, dne_pendulum_final_state,
 * dne_maze_final_state and dne_get_profile follow it.  dne_mujoco_ga_promote makes the theta of descriptor j the new parent j, for all
 * T_new <= T_max at once and from the bank as it was: a kept parent may move and two descriptors may name one source.
 * dne_mujoco_ga_parents returns T (-1 on another kind), dne_mujoco_ga_get_parent copies one parent [P] out.
 * Refused by name, with the bank left bit for bit as it was: another kind, a call before dne_mujoco_ga_reserve, no noise table,
 * (evaluation) no maze loaded, statistics unset, env_seed NULL on the pendulum, T outside [1, T_max], n outside [1, max_members], a parent
 * on an empty bank, parent >= T, parent < -1, a root without an index, the kept form in an evaluation, idx + P past the table, an empty
 * chain or chain_offsets[0] != 0, a missing buffer, tslimit <= 0.  None of these reads or writes the base slots or dne_set_members' members.
 * The *_host calls are the same header on the CPU (no handle, no GPU; kind 6 or 7, hidden 64 / 128 / 256, n_out as dne_*_num_params takes
 * it): the H + H + O column scales of the slice at idx0, the theta of one genome, and of n descriptors -- the kept form included -- against a
 * host bank [T][P] (NULL when T == 0); errors through dne_last_error(NULL). */
int dne_mujoco_ga_reserve(dne_handle *h, int T_max);
int dne_mujoco_ga_build(dne_handle *h, int T, const int32_t *chain_offsets /*T+1*/, const int64_t *seeds, const float *powers);
int dne_mujoco_ga_eval(dne_handle *h, int n, const int32_t *parent, const int64_t *idx, const float *power, const uint32_t *env_seed /*n or NULL*/,
                       int tslimit, float *returns, float *signreturns /*or NULL*/, int32_t *lengths);
int dne_mujoco_ga_promote(dne_handle *h, int T_new, const int32_t *parent, const int64_t *idx, const float *power);
int dne_mujoco_ga_parents(dne_handle *h);
int dne_mujoco_ga_get_parent(dne_handle *h, int j, float *out /*P*/);
int dne_mujoco_ga_colscale_host(const float *noise, size_t count, int kind, int hidden, int n_out, int64_t idx0, float *out /*2 hidden + n_out*/);
int dne_mujoco_ga_theta_host(const float *noise, size_t count, int kind, int hidden, int n_out, const int64_t *seeds, const float *powers, int nseeds,
                             float *out /*P*/);
int dne_mujoco_ga_members_host(const float *noise, size_t count, int kind, int hidden, int n_out, const float *bank /*[T][P]*/, int T,
                               const int32_t *parent, const int64_t *idx, const float *power, int n, float *out /*[n][P]*/);

/* ---- novelty on the hard maze (csrc/maze_novelty.h) -------------------------------------------
 * A behaviour characterisation is one float32 point (x, y): a navigator's final position.  nses.py:12-32 on such points: for member p and
 * archive point a, d = sqrt(dx*dx + dy*dy) in double with dx = (double)ax - (double)px (unfused, correctly rounded sqrt); novelty = the
 * kk = min(k, archive size) smallest d, ordered by (isnan, value, archive slot), added one by one in that order into a double that starts at
 * 0.0, divided by kk.  Every number sorts before every NaN; ties go to the lower slot.
 * The archive is a device buffer of float pairs in insertion order (the slot is the position); it grows geometrically.  Appends, clears and
 * scoring are ordered on the engine's stream.  xy == NULL means the first n members of the last evaluation, read on the device where
 * k_maze_rollout left them (1 <= n <= the members the last evaluation ran, as dne_maze_final_state); a host xy takes any n >= 1.
 * Refused by name: an engine of another kind, an empty archive, k < 1, k > DNE_MAZE_NOVELTY_KMAX, n < 1, cap below the archive's size.  A
 * refused call leaves the archive as it was.  The byte-trajectory calls above (dne_archive_*, dne_novelty*) keep refusing this kind.
 * dne_maze_archive_size returns the number of points (-1 on an engine of another kind); dne_maze_archive_get copies them out in order.
 * dne_maze_novelty_host is the same header on the CPU: no handle, no GPU, any k >= 1.
 * dne_maze_novelty_last_ms: k_maze_novelty of the last dne_maze_novelty between two device events, in milliseconds (-1 before the first). */
#define DNE_MAZE_NOVELTY_KMAX 32
int dne_maze_archive_append(dne_handle *h, const float *xy /*[n][2], or NULL*/, int n);
int dne_maze_archive_clear(dne_handle *h);
int dne_maze_archive_size(dne_handle *h);
int dne_maze_archive_get(dne_handle *h, float *xy /*[cap][2]*/, int cap);
int dne_maze_novelty(dne_handle *h, const float *xy /*[n][2], or NULL*/, int n, int k, double *out /*[n]*/);
int dne_maze_novelty_host(const float *xy, int n, const float *archive /*[narch][2]*/, int narch, int k, double *out);
double dne_maze_novelty_last_ms(dne_handle *h);
/* Pool novelty (GA-NS): member p of the n members is scored against the archive's A points at combined slots 0 .. A - 1
 * followed by the n members at combined slots A .. A + n - 1, the combined slot A + p left out -- by index, not by value.  Distances, keys and
 * the sequential sum are the ones above; the order is (key, combined slot), so an archive point comes before a population point at the same
 * distance; kk = min(k, A + n - 1).  A NaN member gets a NaN novelty.  xy == NULL reads the last evaluation's first n members on the device
 * (dne_maze_final_state's rule for n); a host xy takes any n >= 1.  dne_maze_novelty_pool_host is the same header on the CPU (narch may be
 * 0, any k >= 1).  dne_maze_archive_append_members appends the final positions of the last evaluation's members members[0 .. count - 1], in
 * that order, device to device (k_maze_archive_gather); indices may repeat.
 * Refused by name, the archive left as it was: an engine of another kind, k < 1, k > DNE_MAZE_NOVELTY_KMAX, n < 1, an empty pool (n = 1 and
 * A = 0), the NULL form beyond the last evaluation's members; for the gather count < 1 and an index outside the last evaluation's members.
 * dne_maze_novelty_last_ms reports the scoring kernel of the last dne_maze_novelty or dne_maze_novelty_pool. */
int dne_maze_novelty_pool(dne_handle *h, const float *xy /*[n][2], or NULL*/, int n, int k, double *out /*[n]*/);
int dne_maze_novelty_pool_host(const float *xy, int n, const float *archive /*[narch][2]*/, int narch, int k, double *out);
int dne_maze_archive_append_members(dne_handle *h, const int32_t *members /*[count]*/, int count);

/* ---- novelty over final states on a dense policy (DNE_KIND_DENSE; csrc/dense_novelty.h) ------
 * The behaviour characterisation (BC) of a member is D float32 values of its final state record (dne_dense_final_state's doubles), one
 * round-to-nearest cast each, NaN and +-inf passing through: the maze D = 2 (x, y) -- MazeFinalState; the cart-pole D = 4 (x, x_dot, theta,
 * theta_dot); the pendulum D = 2 (theta, theta_dot).  dne_dense_bc_dim returns D, dne_dense_bc copies out the BCs of the last evaluation's
 * first n members (dne_dense_final_state's rule for n).  Novelty is the contract above with D coordinates: d = sqrt(s), s = d_0 * d_0, then
 * s = s + d_i * d_i for i ascending with d_i = (double)a_i - (double)p_i, unfused; the order (isnan, value, archive slot); the kk = min(k,
 * archive size) first distances added one by one into a double from 0.0, divided by kk.  For D = 2 it is dne_maze_novelty's bit for bit.
 * The archive is a device buffer of D floats a point in insertion order; appends, clears and scoring are ordered on the engine's stream.
 * bc == NULL means the first n members of the last evaluation (dne_eval_members, dne_es_eval or dne_dense_ga_eval), device to device.
 * Refused by name, the archive left as it was: an engine of another kind, n < 1, the NULL form beyond the last evaluation's members, an empty
 * archive for a novelty call, k < 1, k > DNE_DENSE_NOVELTY_KMAX, a missing output buffer, cap below the archive's size.  The dne_maze_*
 * calls above keep refusing this kind.  dne_dense_novelty_last_ms: k_dense_novelty of the last dne_dense_novelty between two device events,
 * in milliseconds (-1 before the first).  dne_dense_novelty_host (D 2 or 4, any k >= 1) and dne_dense_bc_host (rec [n][S] of env_kind) are
 * the same header on the CPU: no handle, no GPU, errors through dne_last_error(NULL). */
#define DNE_DENSE_NOVELTY_KMAX DNE_MAZE_NOVELTY_KMAX
int dne_dense_bc_dim(dne_handle *h);
int dne_dense_bc(dne_handle *h, int n, float *bc /*[n][D]*/);
int dne_dense_archive_append(dne_handle *h, const float *bc /*[n][D], or NULL*/, int n);
int dne_dense_archive_clear(dne_handle *h);
int dne_dense_archive_size(dne_handle *h);
int dne_dense_archive_get(dne_handle *h, float *bc /*[cap][D]*/, int cap);
int dne_dense_novelty(dne_handle *h, const float *bc /*[n][D], or NULL*/, int n, int k, double *out /*[n]*/);
double dne_dense_novelty_last_ms(dne_handle *h);
int dne_dense_novelty_host(const float *bc, int n, const float *archive /*[narch][D]*/, int narch, int D, int k, double *out);
int dne_dense_bc_host(int env_kind, const double *rec /*[n][S]*/, int n, float *bc /*[n][D]*/);
/* Pool novelty on a dense policy (GA-NS): section 12c's contract with the point above.  Member p of the n members is
 * scored against the archive's A points at combined slots 0 .. A - 1 followed by the n members at combined slots A .. A + n - 1, the combined
 * slot A + p left out -- by index, not by value.  Distances, keys and the sequential sum are dne_dense_novelty's; the order is (key, combined
 * slot), so an archive point comes before a population point at the same distance; kk = min(k, A + n - 1).  A NaN member gets a NaN novelty.
 * bc == NULL reads the BCs of the last evaluation's first n members on the device (dne_dense_final_state's rule for n), and those n are the
 * population; a host bc takes any n >= 1.  dne_dense_novelty_pool_host is the same header on the CPU (narch may be 0 and archive NULL then,
 * any k >= 1, D 2 or 4).  dne_dense_archive_append_members appends the BCs of the last evaluation's members members[0 .. count - 1], in that
 * order, device to device (k_dense_archive_gather); indices may repeat and are checked before anything is launched.
 * Refused by name, the archive left as it was: an engine of another kind, n < 1, the NULL form beyond the last evaluation's members (or before
 * any), k < 1, k > DNE_DENSE_NOVELTY_KMAX, an empty pool (n = 1 and A = 0), a missing output buffer; for the gather count < 1 and an index
 * outside the last evaluation's members; for the host twin a missing buffer and D outside {2, 4}.  dne_maze_novelty_pool and
 * dne_maze_archive_append_members keep refusing this kind.  dne_dense_novelty_last_ms reports the scoring kernel of the last
 * dne_dense_novelty or dne_dense_novelty_pool. */
int dne_dense_novelty_pool(dne_handle *h, const float *bc /*[n][D], or NULL*/, int n, int k, double *out /*[n]*/);
int dne_dense_novelty_pool_host(const float *bc, int n, const float *archive /*[narch][D], or NULL with narch 0*/, int narch, int D, int k, double *out);
int dne_dense_archive_append_members(dne_handle *h, const int32_t *members /*[count]*/, int count);

/* ---- Deep-GA on the hard maze (csrc/maze_ga.h) -----------------------------------------------
 * gpu_implementation/ga.py on SimpleClassifier.  A genome is (idx0, (idx1, power1), ...) as seeds[] / powers[] (powers[0] is not read):
 * theta_p = fl(noise[idx0 + p] * scale_by[p]), then per mutation, in order, theta_p = theta_p + fl(power_j * noise[idx_j + p]), never fused.
 * The parents live in a bank on the device (T of them, at most max_members), apart from the base slots of dne_set_theta, which no call here
 * reads or writes.  A member descriptor (parent, idx, power) against the bank is one of
 *   root   parent == -1, idx >= 0      theta_p = fl(noise[idx + p] * scale_by[p]); power is not read
 *   child  0 <= parent < T, idx >= 0   theta_p = bank[parent][p] + fl(power * noise[idx + p])   (power 0: the parent evaluated again)
 *   kept   0 <= parent < T, idx < 0    bank[parent] bit for bit: dne_maze_ga_promote only
 * dne_maze_ga_build fills the bank with T parents from their genomes (chain_offsets [T + 1] into seeds / powers, from 0).
 * dne_maze_ga_eval runs one episode per root / child member in one k_maze_rollout launch; dne_maze_final_state, dne_maze_novelty(xy = NULL)
 * and dne_get_profile follow it as they follow any evaluation.  dne_maze_ga_promote makes the theta of descriptor j the new parent j, for
 * all T_new at once, reading the old bank and writing the other half of a double buffer: a kept parent may change its index and two
 * descriptors may name one source.  dne_maze_ga_parents returns T (-1 on another kind), dne_maze_ga_get_parent copies one parent out.
 * All calls are ordered on the engine's stream.  Refused by name, the bank staying as it was: an engine of another kind; no init scale; no
 * noise table (for an evaluation: no walls); parent >= T, or any parent >= 0 on an empty bank; the kept form in an evaluation; idx + 498
 * past the table; n or T outside 1 .. max_members; an empty chain.  dne_ga_* keep refusing this kind.
 * dne_maze_ga_theta_host / dne_maze_ga_members_host are the same header on the CPU (no handle, no GPU): the theta of one genome, and of n
 * descriptors (all three forms) against a host bank [T][498]. */
int dne_maze_ga_set_init_scale(dne_handle *h, const float *scale_by, size_t n /*498*/);
int dne_maze_ga_build(dne_handle *h, int T, const int32_t *chain_offsets /*T+1*/, const int64_t *seeds, const float *powers);
int dne_maze_ga_eval(dne_handle *h, int n, const int32_t *parent, const int64_t *idx, const float *power, int tslimit, float *returns,
                     float *signreturns /*or NULL*/, int32_t *lengths);
int dne_maze_ga_promote(dne_handle *h, int T_new, const int32_t *parent, const int64_t *idx, const float *power);
int dne_maze_ga_parents(dne_handle *h);
int dne_maze_ga_get_parent(dne_handle *h, int j, float *out /*498*/);
int dne_maze_ga_theta_host(const float *noise, size_t count, const float *scale_by, const int64_t *seeds, const float *powers, int nseeds,
                           float *out /*498*/);
int dne_maze_ga_members_host(const float *noise, size_t count, const float *scale_by, const float *bank /*[T][498]*/, int T,
                             const int32_t *parent, const int64_t *idx, const float *power, int n, float *out /*[n][498]*/);

#ifdef __cplusplus
}
#endif
#endif
