// plan.h -- which kernels a lock-step launches, decided on the host from plain values: no HIP, no kernels, no handle.
// Knobs (the DNE_* tuning variables, one table) + PlanFacts (what the member set and the engine's buffers allow) + the active count
// -> StepPlan (the regime of a burst: the lock-steps between two compactions of the active list) -> WindowPlan (every choice the
// launchers of engine.hip make for one window of that burst).  dne_debug_plan walks the same functions without a device.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/dne_hip.h"

// ------------------------------------------------------------------------------- knobs
// Every scheduling and tuning value dne_create takes from the environment (measurement only; none is part of the contract).  The
// initialisers are the defaults tools/knob_table.py prints; where a default differs per engine kind knobs_from_env sets it.
struct Knobs {
    int ga_sort = 1;
    int conv_fused = 1, conv_fused_min = 129;
    int nsub_fixed = 0, nsub_full = 4, nsub_mid = 4;
    int fc_tail_max = 96, fc_quad_max = 4, fc_tailk_max = 32;
    int dbg_skip = 0, dbg_immortal = 0;
    int tt_enable = 1;
    int head_threads = 320, render_threads = 512, band_threads = 512;
    int tail_fused_max = 200;
    int fc_pairs = 2;
    int conv1_fpw = 8;
    int conv_split_max = 32, conv12t_max = 64, conv_split_mid = 256;
    int fc2_min_total = 800;
    int spec_max = 4, spec_bands = 7, spec_conv1 = 1;
    int fc_duo = 1, duo_lag = 0, fc_prio = 3, duo_sweep = 2, duo_sync = 1, duo_fat = 1;
    int ring_on = 1, ring_min = 1000, ring_pre = 1;
    int sub_render_fused = 0;
    int burst = 32, burst_tail = 16;
    int duo_grid = 0;
    int fc_sub = 1, fc_sub_min = 97, fc_sub_max = 320, fc_sub_nsub = 2, fc_sub_spw = 0, fc_sub_prio = 0, fc_sub_grid = 512, fc_sub_head = 1;
    int conv2_ref_fpw = 8;
    int duo_solo_below = 1500, duo_head_fused = 0;
    int out_lds_kb = 0;
    int fc_duo_min = 451;
    int render_bands = 8, render_wg_max = 512;
    int fc_chain_min = 1 << 30;
    int fc_grid = 512;
    int conv1_shared = 1;
    int ga_materialize = 0;
    int lfc_cols_max = 96, lfc_pad = 2;
    int fc_rb = 4;
    int ref_dedup = 1;
};

struct KnobRow { const char *env; int lo, hi; int Knobs::*field; const char *text; };

// one row per knob: the variable, the range its value is clamped to, the field, what it selects (DESIGN.md section 11 is this table)
static const KnobRow KNOBS[] = {
    {"DNE_GA_SORT", 0, 1, &Knobs::ga_sort, "evaluate a generation's children grouped by parent"},
    {"DNE_CONV_FUSED", 0, 1, &Knobs::conv_fused, "conv1 + conv2 in one kernel (k_conv12: one workgroup per member, y1 stays in LDS) from DNE_CONV_FUSED_MIN members"},
    {"DNE_CONV_FUSED_MIN", 1, 1 << 20, &Knobs::conv_fused_min, "conv1 + conv2 in one kernel from this many members"},
    {"DNE_NSUB", 1, 4, &Knobs::nsub_fixed, "windows of every burst, whatever the active count (unset: by the active count)"},
    {"DNE_NSUB_FULL", 1, 4, &Knobs::nsub_full, "windows at full width (>= 1900 active groups)"},
    {"DNE_NSUB_MID", 1, 4, &Knobs::nsub_mid, "windows between 800 and 1899 active groups"},
    {"DNE_FC_TAIL_MAX", 1, 1 << 20, &Knobs::fc_tail_max, "windows of up to this many groups take the latency-bound fc kernels (k_fc_quad / k_fc_tail / k_fc_cols), wider ones the streaming kernels"},
    {"DNE_FC_QUAD_MAX", 0, 1 << 20, &Knobs::fc_quad_max, "up to this many groups per window the 64-workgroups-per-group fc (k_fc_quad); above it k_fc_tail"},
    {"DNE_FC_TAILK_MAX", 0, 1 << 20, &Knobs::fc_tailk_max, "up to this many groups per window k_fc_tail (16 workgroups per group), above it k_fc_cols (4 lean ones)"},
    {"DNE_DEBUG_SKIP", 0, 7, &Knobs::dbg_skip, "bitmask (timing experiments only): 1 conv1, 2 conv2, 4 render"},
    {"DNE_DEBUG_IMMORTAL", 0, 1, &Knobs::dbg_immortal, "(timing experiments only): every member lives until tslimit -- a lock-step keeps its width"},
    {"DNE_TAIL_TABLE", 0, 1, &Knobs::tt_enable, "with at most TT_MAX members left, all in one window, the member descriptors ride in the kernel arguments"},
    {"DNE_HEAD_THREADS", 256, 320, &Knobs::head_threads, "320 = the policy head's four waves + a fifth that steps the emulator for every action meanwhile; 256 = one lane steps it afterwards"},
    {"DNE_RENDER_THREADS", 256, 1024, &Knobs::render_threads, "threads per k_env_render workgroup above 192 members (one workgroup per member).  Round 5: 512 -- beside k_fc_ring a generation takes 216.8 instead of 223.1 ms same-box (768: 217.2, 1024: 235.3); rounds 1-4: 256 (beside k_fc_duo 512 measured +1 %)"},
    {"DNE_BAND_THREADS", 256, 1024, &Knobs::band_threads, "tail: threads of each of a frame's DNE_RENDER_BANDS workgroups"},
    {"DNE_TAIL_FUSED_MAX", 0, 1 << 20, &Knobs::tail_fused_max, "up to this many active groups (all windows) k_out + k_env_logic + k_env_render run as one kernel"},
    {"DNE_FC_PAIRS", 1, 2, &Knobs::fc_pairs, "ES full-width fc: antithetic pairs per work item (1 = k_fc<2>)"},
    {"DNE_CONV1_FPW", 1, 8, &Knobs::conv1_fpw, "reference pass: frames per conv1 workgroup (1, 2, 4, 8)"},
    {"DNE_CONV_SPLIT_MAX", 0, 1 << 20, &Knobs::conv_split_max, "members up to which the convolutions use their finest split"},
    {"DNE_CONV12T_MAX", 0, 1 << 20, &Knobs::conv12t_max, "members up to which conv1 -> conv2 is one launch of four workgroups per member (0 = off)"},
    {"DNE_CONV_SPLIT_MID", 0, 1 << 20, &Knobs::conv_split_mid, "... their middle split: conv1 over 4 workgroups up to this many members, conv2 over 2 up to twice as many"},
    {"DNE_FC2_MIN", 2, 1 << 30, &Knobs::fc2_min_total, "k_fc2 from this many active groups upwards"},
    {"DNE_SPEC_MAX", 0, 64, &Knobs::spec_max, "a single window of up to this many members (2 antithetic pairs; round 2: 8 -- the faster tail kernels of round 3 beat speculation at 4 pairs, 47 vs 56 us) steps speculatively -- every action's outcome is worked out under the forward pass; 0 = off"},
    {"DNE_SPEC_BANDS", 1, 12, &Knobs::spec_bands, "256-thread workgroups per candidate frame"},
    {"DNE_SPEC_CONV1", 0, 1, &Knobs::spec_conv1, "conv1 of every candidate stack in the launch that picks the action"},
    {"DNE_FC_DUO", 0, 1, &Knobs::fc_duo, "table-ordered fc (k_unit_order + k_fc_duo + k_out) from DNE_FC_DUO_MIN active groups"},
    {"DNE_DUO_LAG", 0, 64, &Knobs::duo_lag, "extra row batches by which the second unit of a duo trails the first"},
    {"DNE_FC_PRIO", 0, 3, &Knobs::fc_prio, "s_setprio of k_fc_duo's waves (0-3)"},
    {"DNE_DUO_SWEEP", 0, 2, &Knobs::duo_sweep, "(0 = off): the four waves of a k_fc_duo workgroup walk one table timeline (1: two units per wave only, 2: also one unit per wave)"},
    {"DNE_DUO_SYNC", 1, 8, &Knobs::duo_sync, "row blocks per barrier of the sweep (1-8)"},
    {"DNE_DUO_FAT", 0, 1, &Knobs::duo_fat, "k_fc_duo with a register footprint past 256 per lane = at most one of its workgroups per CU (it streams as fast from one), so the other windows' kernels always find room beside it"},
    {"DNE_FC_RING", 0, 2, &Knobs::ring_on, "(round 5): k_fc_ring instead of k_fc_duo -- the workgroup's noise rows through an LDS ring filled by LDS-DMA, the base rows from a column-permuted copy of the fc matrix; 1: from DNE_DUO_SOLO_BELOW active pairs (1500) upwards, 2: in the whole k_fc_duo range (measured slower in the sparse part: 239 vs 233 ms), 0: k_fc_duo everywhere"},
    {"DNE_RING_MIN", 0, 1 << 30, &Knobs::ring_min, "k_fc_ring needs this many active pairs on the rank whatever their density (below, its workgroups -- eight units, one per CU -- no longer fill the chip: a 625-pair share measured 61.6 ms per generation on the ring against 57.8 on k_fc_duo, profiles/r06_shard_ab.jsonl)"},
    {"DNE_RING_PRE", 0, 1, &Knobs::ring_pre, "0 = the ring multiplies every row by sigma itself (rounds 5-6a); 1 = it streams the table scaled by the evaluation's sigma (k_scale_table)"},
    {"DNE_SUB_RENDER_FUSED", 0, 1, &Knobs::sub_render_fused, "(round 6, VERDICT item 1c): behind the sub-slice fc the policy head, the emulator AND the renderer in one launch (k_tail_step<.., true>, 1024 threads per member): three launches per window and lock-step instead of four"},
    {"DNE_BURST", 1, 256, &Knobs::burst, "lock-steps between two compactions of the active list (a host round trip each) above DNE_FC_TAIL_MAX active groups (round 4: 32, 16 before; 24 / 32 / 48 measured -0.5 .. -0.9 %, 8 +2.3 %, 64 +0.2 %)"},
    {"DNE_BURST_TAIL", 1, 256, &Knobs::burst_tail, "... with at most DNE_FC_TAIL_MAX groups alive (the tail measured indifferent)"},
    {"DNE_DUO_GRID", 0, 1 << 16, &Knobs::duo_grid, "persistent grid of k_fc_duo (0 = fc_grid)"},
    // measured (tools/ga_lockstep_profile.py, tools/ab_inproc.py --pairs 312 / 625): Deep-GA children 97 .. 320 alive, four windows
    // at wave priority 0 (round 6; two at 3 before: 1.02-1.05 vs 0.98-1.00 M env-steps/s same-box; five / six windows 0.91-0.94), a grid of 512
    // workgroups; ES pairs 97 .. 450 alive, three windows, the whole launch resident; above those widths the streaming kernels win
    {"DNE_FC_SUB", 0, 2, &Knobs::fc_sub, "(ES 2, GA 1): the sub-slice fc (k_fc_sub: one wave per 128 / 120-row chain) in the mid range -- 0 off, 1 GA children (materialised), 2 also ES pairs"},
    {"DNE_FC_SUB_MIN", 1, 1 << 30, &Knobs::fc_sub_min, "active groups (all windows) from which the sub-slice fc runs"},
    {"DNE_FC_SUB_MAX", 1, 1 << 30, &Knobs::fc_sub_max, "... and up to which (450 for ES pairs, 320 for GA children)"},
    {"DNE_FC_SUB_NSUB", 1, 4, &Knobs::fc_sub_nsub, "windows of that regime (ES 3, GA 4 since round 6)"},
    {"DNE_FC_SUB_SPW", 0, 8, &Knobs::fc_sub_spw, "sub-slices per wave (1, 2, 4, 8; 0 = by width)"},
    {"DNE_FC_SUB_PRIO", 0, 3, &Knobs::fc_sub_prio, "s_setprio of k_fc_sub's waves (ES 0: the regime is bound by a window's chain of small kernels, they must not starve; GA: 0 since round 6, 3 on its bounded grid before)"},
    {"DNE_FC_SUB_GRID", 1, 1 << 20, &Knobs::fc_sub_grid, "workgroups of k_fc_sub at most, 4 waves each (GA 512 = two waves per SIMD; ES: the whole launch resident)"},
    {"DNE_FC_SUB_HEAD", 0, 1, &Knobs::fc_sub_head, "policy head + emulator step in one launch (k_tail_step) behind k_fc_sub instead of k_out + k_env_logic"},
    {"DNE_CONV2_REF_FPW", 1, 8, &Knobs::conv2_ref_fpw, "reference frames per conv2 workgroup (8, 4, or 1 = the lock-step kernel)"},
    {"DNE_DUO_SOLO_BELOW", 0, 1 << 30, &Knobs::duo_solo_below, "with fewer active groups (all windows) every wave takes one unit instead of two (sparse table: little to share, and twice the waves)"},
    {"DNE_DUO_HEAD_FUSED", 0, 1, &Knobs::duo_head_fused, "behind k_fc_duo the policy head and the emulator step share a launch (k_tail_step) instead of k_out + k_env_logic; same-box A/B: 402.7 ms fused, 403.3 separate, 399.8 separate with k_out at two workgroups per CU -> off"},
    {"DNE_OUT_LDS_KB", 0, 64, &Knobs::out_lds_kb, "an LDS reservation that bounds k_out's workgroups per CU behind k_fc_ring / k_fc_duo: the launch asks for this much when it is more than the staged output weights need (39 KB for a pair at 18 actions: four workgroups per CU; 64 KB: two)"},
    {"DNE_FC_DUO_MIN", 2, 1 << 30, &Knobs::fc_duo_min, "table-ordered fc from this many active groups (round 4: 451, right above the sub-slice fc's range; 800 before -- with one k_fc_duo workgroup per CU a 625-pair share takes 84.5 instead of 88.4 ms per generation)"},
    {"DNE_RENDER_BANDS", 1, 84, &Knobs::render_bands, "tail: workgroups per frame (1 = render inside k_tail_step)"},
    {"DNE_RENDER_WG_MAX", 1, 1 << 20, &Knobs::render_wg_max, "... halved until members x bands fits this many workgroups"},
    {"DNE_FC_CHAIN_MIN", 1, 1 << 30, &Knobs::fc_chain_min, "windows of at least this many groups wait for the previous window's fc before they start theirs (anti-phase; off by default, free-running measured faster)"},
    {"DNE_FC_GRID", 1, 1 << 16, &Knobs::fc_grid, "persistent grid of the streaming fc kernels (workgroups at most)"},
    {"DNE_CONV1_SHARED", 0, 1, &Knobs::conv1_shared, "reference-pass conv1 with eight members sharing a frame in LDS"},
    {"DNE_GA_MATERIALIZE", 0, 1, &Knobs::ga_materialize, "GA children written out once per generation, the streaming fc then reads plain rows (default: on for GA engines)"},
    {"DNE_LFC_COLS_MAX", 0, 1 << 20, &Knobs::lfc_cols_max, "LargeModel windows of up to this many members use the column-split fc"},
    {"DNE_LFC_PAD", 0, 2, &Knobs::lfc_pad, "LargeModel's streamed fc with a padded register footprint -- 1: at most two of its workgroups per CU, 2: one (0: as many as fit, five); same-box 282.5 / 285.2 / 291.2 k env-steps/s at 0 / 1 / 2"},
    {"DNE_FC_RB", 2, 8, &Knobs::fc_rb, "rows per batch of the streaming fc kernels (2, 4, 8; the LargeModel's default is 8: measured 8 % faster than 4)"},
    {"DNE_REF_DEDUP", 0, 1, &Knobs::ref_dedup, "reference pass on the batch's unique conv rows when the batch has few enough (ref_index.h: ref_dedup_pays); 0 = no tables are allocated, every batch takes the dense kernels"},
};

// ES-like kinds: ESAtariPolicy and the GPU tree's ModelVirtualBN -- the same network, virtual batch norm over a reference batch, antithetic
// pairs over one theta, the ES reduce and optimizer; they differ only in the flat layout
static inline bool es_like(int kind) { return kind == DNE_KIND_ES || kind == DNE_KIND_ES_VBN; }

// per-kind defaults, then the environment (every value clamped to what the kernels support), then the values only some kernels exist for.
// max_spec_actions: the widest action set the speculative tail's candidate arrays hold.
static inline Knobs knobs_from_env(int kind, int n_actions, int max_spec_actions) {
    Knobs k;
    if (es_like(kind)) { k.fc_sub = 2; k.fc_sub_max = 450; k.fc_sub_nsub = 3; k.fc_sub_grid = 1 << 20; }
    else { k.fc_sub_nsub = 4; k.ga_materialize = 1; }
    if (kind == DNE_KIND_GA_LARGE) k.fc_rb = 8;
    for (const KnobRow &r : KNOBS)
        if (const char *e = getenv(r.env)) k.*r.field = std::max(r.lo, std::min(r.hi, atoi(e)));
    auto wg_size = [](int v) { return v >= 1024 ? 1024 : v >= 512 ? 512 : 256; };   // the renderer needs >= 210 threads, whole waves
    k.head_threads = k.head_threads >= 320 ? 320 : 256;
    k.render_threads = wg_size(k.render_threads);
    k.band_threads = wg_size(k.band_threads);
    if (k.fc_sub_spw != 1 && k.fc_sub_spw != 2 && k.fc_sub_spw != 4 && k.fc_sub_spw != 8) k.fc_sub_spw = 0;
    if (es_like(kind)) k.ga_materialize = 0;   // ES members are antithetic pairs over one theta: nothing to write out
    if (n_actions > max_spec_actions) k.spec_max = 0;
    return k;
}

// ------------------------------------------------------------------------------- facts
// what the planner reads beyond the knobs: the engine kind, what dne_set_members found out about the member set, which buffers exist
using PlanFacts = dne_plan_facts;
static inline bool is_large(const PlanFacts &f) { return f.kind == DNE_KIND_GA_LARGE; }

// ------------------------------------------------------------------------------- the regime of a burst
// The empty plan is what every caller outside an evaluation gets (dne_act): one window, k_fc or the column-split kernels.
struct StepPlan {
    int nsub = 1;            // windows the active list is cut into, each on its own stream
    bool sub = false;        // every window: k_fc_sub (one wave per sub-slice chain), the head folds its chain sums
    bool duo = false;        // windows above fc_tail_max groups: table-ordered units (k_unit_order + k_fc_duo + k_out) ...
    bool duo_solo = false;   // ... one unit per wave instead of two (sparse table: little to share, and twice the waves)
    bool ring = false;       // ... k_fc_ring instead of k_fc_duo (the windows' convolutions leave activated y2)
    bool ring_scaled = false; // ... its DMA source the table scaled by the evaluation's sigma (noise_pre)
    bool fc2 = false;        // else k_fc2 (two pairs per work item share the base rows), else k_fc
    bool lpair = false;      // LargeModel, antithetic pairs, windows above lfc_cols_max MEMBERS: k_lfc_pair (a pair's eps and theta rows fetched once)
};

// The regime of a burst that starts with `total` active groups of `gsize` members.  One global list of active groups, compacted every burst; within a burst
// the list is cut into nsub equal windows, each stepped on its own stream, so that while one window streams its noise slices (HBM) the others run their MFMA
// convolutions and emulator frames.  whole_eval: the same conditions classify an evaluation by the width it STARTS with (which launches carry profiling
// events, dne_profile.fc_full_kind); the two terms that differ between the two uses are marked.
static inline StepPlan plan_step(const Knobs &k, const PlanFacts &f, int total, int gsize, bool whole_eval = false) {
    const bool es = es_like(f.kind), large = is_large(f), pairs = es && gsize == 2;
    StepPlan p;
    // the sub-slice fc's range: GA children written out (plain rows), optionally ES pairs (DNE_FC_SUB=2); never the LargeModel
    if (!large && f.has_y3s && total >= k.fc_sub_min && total <= k.fc_sub_max)
        p.sub = es ? k.fc_sub >= 2 && gsize == 2 && total < k.fc_duo_min : k.fc_sub >= 1 && gsize == 1 && f.members_materialized;
    // nsub follows the active count (tools/kbench.py sweeps): k_fc2 wants 3 windows at full width and 4 in the upper mid range; below
    // ~400 groups the windows are sized to fit the column-split tail kernels (<= fc_tail_max groups each); one when only a handful of episodes are left
    int n = total >= 1900 ? k.nsub_full : total >= k.fc2_min_total ? k.nsub_mid : total > 4 * k.fc_tail_max ? 3
          : total >= 48 ? std::max(2, (total + k.fc_tail_max - 1) / k.fc_tail_max) : 1;
    if (p.sub) n = k.fc_sub_nsub;
    if (k.nsub_fixed > 0) n = k.nsub_fixed;
    n = std::min(n, (int)f.n_streams);
    p.nsub = std::max(1, std::min(n, total));
    // a burst inside the sub-slice fc's range runs no k_fc2; an evaluation that starts there with k_fc2 enabled at that width
    // (DNE_FC2_MIN lowered into the range) still counts as a k_fc2 evaluation, whose profiled launches are the k_fc2 ones
    p.fc2 = k.fc_pairs == 2 && pairs && f.uniform_base && total >= k.fc2_min_total && (whole_eval || !p.sub);
    // table-ordered units (never inside the sub-slice fc's range, which ends below fc_duo_min).  k_unit_order ranks a window's keys
    // in LDS: a burst whose windows are too long for it falls back to k_fc2 / k_fc; the evaluation's kind ignores that bound
    const bool order_fits = (size_t)4 * ((total + p.nsub - 1) / p.nsub) * sizeof(long long) <= 160 * 1024;
    p.duo = !large && k.fc_duo && pairs && total >= k.fc_duo_min && (whole_eval || order_fits);
    p.duo_solo = total < k.duo_solo_below;
    // the ring's range: pairs as dense in their stretch of the table as DNE_DUO_SOLO_BELOW (1500) pairs over the whole table, and enough of them to
    // fill the chip (DNE_RING_MIN) -- at one GPU "1500 of 2500 active", on a rank of two with its own half of the table "1000 of 1250"
    const bool dense = (double)total * f.dense_scale >= (double)k.duo_solo_below && total >= k.ring_min;
    p.ring = p.duo && f.has_theta_perm && f.antithetic_slot0 && k.duo_sweep && (k.ring_on > 1 || dense) && (dense || k.duo_sweep > 1);
    p.ring_scaled = p.ring && k.ring_pre && f.pair_sigma_uniform && f.has_scaled_table;   // (the evaluation started at least as wide and filled the copy)
    // the LargeModel's pairs (dne_es_eval over base slot 0): the windows of a burst differ by at most one pair, the widest decides the regime
    p.lpair = large && gsize == 2 && f.antithetic_slot0 && 2 * ((total + p.nsub - 1) / p.nsub) > k.lfc_cols_max;
    return p;
}

// dne_profile.fc_full_kind of an evaluation whose starting width gives plan_step(.., whole_eval = true) = ev
// (one that STARTS in the sub-slice fc's range: its bracketed launches are k_fc_sub's)
static inline int fc_full_kind(const StepPlan &ev) { return ev.lpair ? 6 : ev.ring ? 5 : ev.duo ? 3 : ev.fc2 ? 2 : ev.sub ? 4 : 1; }

// lock-steps until the next compaction of the active list
static inline int burst_length(const Knobs &k, int total) { return total <= k.fc_tail_max ? k.burst_tail : k.burst; }

// tail table: the member descriptors ride in the kernel arguments once all the active groups are one window (never the LargeModel's)
static inline bool tail_table_allowed(const Knobs &k, const PlanFacts &f, int total, int gsize) {
    return k.tt_enable && !is_large(f) && plan_step(k, f, total, gsize).nsub == 1;
}

// ------------------------------------------------------------------------------- one window of a burst
struct Window { int lo, cnt; };
// window s of nsub over `total` active groups: the one copy of the cut
static inline Window window(int total, int nsub, int s) {
    const int lo = (int)((long long)total * s / nsub);
    return {lo, (int)((long long)total * (s + 1) / nsub) - lo};
}

using WindowPlan = dne_window_plan;
static inline const char *fc_name(int fc) {
    static const char *const names[] = {"k_lfc_cols", "k_lfc", "k_fc_sub", "k_fc_quad", "k_fc_tail", "k_fc_cols", "k_fc_ring", "k_fc_duo", "k_fc2", "k_fc", "k_lfc_pair"};
    return names[fc];
}
static inline bool is_duo(const WindowPlan &w) { return w.fc == DNE_FC_RING || w.fc == DNE_FC_DUO; }   // table-ordered units: the window has a unit order

// Everything the launchers decide for a window of `cnt` groups in a burst of `total`: the convolution path, the fc kernel and its shape, how the
// policy head, the emulator and the renderer follow.  in_eval = false: dne_act / dne_env_step (p is the empty plan), no fused tail of any kind.
static inline WindowPlan plan_window(const Knobs &k, const PlanFacts &f, const StepPlan &p, int total, int cnt, int gsize, bool in_eval) {
    const bool es = es_like(f.kind), large = is_large(f);
    const int items = cnt * gsize;
    WindowPlan w;
    memset(&w, 0, sizeof(w));
    w.cnt = cnt;
    w.wide = cnt > k.fc_tail_max;
    w.skip = k.dbg_skip;
    if (large) {   // LargeModel: three matrix-core convolutions; few members: one workgroup per 16-channel tile.  Its kernels walk members
        w.conv = DNE_CONV_LARGE;   // (a pair is two of them), so the thresholds of THIS function (s1 / s2, wide, lfc_cols_max) count MEMBERS;
                                   // plan_step's cut into windows and burst_length count groups for every kind, pairs included
        w.s1 = w.s2 = items <= 128 ? 4 : items <= 256 ? 2 : 1;
        w.wide = items > k.fc_tail_max;
    } else {
        w.act2 = p.ring && w.wide;   // the window's fc is k_fc_ring: leave relu(bn2(y2)) instead of y2 (ES pairs only)
        // few members left: several workgroups per member (conv1: 28 position tiles over 4 or 7 workgroups; conv2: 8 over 2 or 4)
        w.s1 = items <= k.conv_split_max ? 7 : items <= k.conv_split_mid ? 4 : 1;
        w.s2 = items <= k.conv_split_max ? 4 : items <= 2 * k.conv_split_mid ? 2 : 1;
        w.conv = k.conv_fused && items >= k.conv_fused_min && !k.dbg_skip ? DNE_CONV_FUSED   // one workgroup per member through both convolutions, y1 stays in LDS
                 : items <= k.conv12t_max && !k.dbg_skip ? DNE_CONV_TAIL4                      // the tail: four workgroups per member through both, no y1 round trip
                                                         : DNE_CONV_SPLIT;                     // k_conv1 + k_conv2
    }
    const bool duo_win = p.duo && w.wide;
    if (large)   // few members: eight workgroups each; antithetic pairs over base slot 0: k_lfc_pair; else one streamed pass per member
        w.fc = items <= k.lfc_cols_max ? DNE_FC_LFC_COLS : gsize == 2 && f.antithetic_slot0 ? DNE_FC_LFC_PAIR : DNE_FC_LFC;
    else if (p.sub) {   // mid range: one wave per sub-slice chain, folded by the head
        w.fc = DNE_FC_SUB;
        // sub-slices per wave: about 8000 waves (one round of the whole machine) whatever the width
        w.sub_spw = k.fc_sub_spw ? k.fc_sub_spw : cnt * k.fc_sub_nsub <= 320 ? 1 : cnt * k.fc_sub_nsub <= 640 ? 2 : cnt * k.fc_sub_nsub <= 1280 ? 4 : 8;
        w.sub_blocks = std::min((32 * cnt / w.sub_spw + 3) / 4, k.fc_sub_grid);
    } else if (!w.wide) {   // latency-bound regime: 4 .. 64 workgroups per group + a separate output-layer kernel
        const bool plain = gsize != 2 && !es && f.members_materialized;   // GA children written out: k_fc_quad / k_fc_tail only
        w.fc = cnt <= k.fc_quad_max ? DNE_FC_QUAD : plain || cnt <= k.fc_tailk_max ? DNE_FC_TAIL : DNE_FC_COLS;
    } else if (p.duo) {   // table-ordered units: adjacent (pair, k-slice) units share their noise rows (ES pairs only: plan_step)
        w.fc = p.ring ? DNE_FC_RING : DNE_FC_DUO;
        w.solo = p.duo_solo;
        w.sweep = k.duo_sweep && (!p.duo_solo || k.duo_sweep > 1);
        w.fat = k.duo_fat;
        w.ring_scaled = p.ring_scaled;
    } else w.fc = p.fc2 ? DNE_FC_FC2 : DNE_FC_FC;   // two pairs per work item share the base rows (ES pairs over one base slot only: plan_step)
    if (in_eval) {
        // fused policy head + emulator (+ render): while all windows together still fit the chip one workgroup per member (the small networks' kernels)
        w.tail = !large && !p.sub && !w.wide && total <= k.tail_fused_max;
        w.spec = w.tail && p.nsub == 1 && k.spec_max > 0 && items <= k.spec_max && items <= k.conv_split_max && !k.dbg_skip;
        w.head_fused = w.tail || (duo_win && k.duo_head_fused) || (p.sub && k.fc_sub_head);   // the fc leaves partial sums: head + emulator in one launch
        // optional: serialise the fc kernels of the windows (anti-phase); off by default, free-running measured faster
        w.chain = p.nsub > 1 && cnt >= k.fc_chain_min;
    }
    // the frames: in the tail each over render_bands workgroups (halved until they fit), or (one band) rendered by the head's own launch
    w.render_bands = w.tail ? k.render_bands : 1;
    while (w.render_bands > 1 && items * w.render_bands > k.render_wg_max) w.render_bands /= 2;
    w.render_fused = w.head_fused && (w.tail ? w.render_bands == 1 : k.sub_render_fused && p.sub && !(k.dbg_skip & 4));
    w.render_wg = w.tail ? k.band_threads : items <= 192 ? 1024 : k.render_threads;
    return w;
}

// dne_act / dne_env_step: the n members as ONE window of single members under the empty plan, outside any evaluation.  dne_debug_plan_act
// answers from this very function, so a test can name the kernels an act at a given width launches before it launches them.
static inline WindowPlan act_window(const Knobs &k, const PlanFacts &f, int n) { return plan_window(k, f, StepPlan{}, n, n, 1, false); }

// (LargeModel: the kind of an evaluation -- 1, or 6 for pairs -- follows lfc_cols_max, the brackets follow w.wide = fc_tail_max.  Both default to 96
// members; set apart, an evaluation of kind 6 / 1 may bracket no launch (DNE_LFC_COLS_MAX=0 with few members) or count a window of k_lfc_cols launches.)
// a profiled evaluation brackets the launches of ONE kernel, the one it starts with (ev = plan_step(.., whole_eval = true)): k_fc_ring's, else k_fc_duo's,
// else k_fc2's, else every window above fc_tail_max groups -- in the latency-bound tail every event packet is a bubble
static inline bool window_profiled(const StepPlan &ev, const StepPlan &p, const WindowPlan &w) {
    return ev.ring ? is_duo(w) && p.ring : ev.duo ? is_duo(w) : ev.fc2 ? p.fc2 : w.wide != 0;
}
