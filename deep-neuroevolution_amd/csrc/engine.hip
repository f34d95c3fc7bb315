// engine.hip -- host side of libdne_hip.so: the C ABI of include/dne_hip.h over the gfx950 kernels in
// env_synth.h / forward.h / reduce.h.  One handle = one HIP device (a main stream + 3 window streams); all state (noise table,
// parent vectors, optimizer moments, frame stacks, emulator RAM, activations) lives in HBM for the
// lifetime of the handle, and a generation only moves (noise_idx, seed) in and (return, length) out.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: librccl.so is opened on demand by dne_comm_init
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <array>
#include <cstdlib>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dne_hip.h"
#include "env_synth.h"
#include "forward.h"
#include "forward_variants.h"
#include "forward_large.h"
#include "reduce.h"
#include "novelty.h"
#include "plan.h"
#include "ref_index.h"
#include "maze.h"
#include "maze_novelty.h"
#include "maze_ga.h"
#include "cartpole.h"
#include "pendulum.h"
#include "mjmaze.h"
#include "step_env.h"
#include "dense.h"
#include "dense_ga.h"
#include "mujoco_ga.h"
#include "dense_novelty.h"
#include "ram_novelty.h"

using namespace dne;

static thread_local std::string g_create_error;

#define HCHECK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) return (h)->fail("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
    } while (0)

// the Atari-only entry points on a hard-maze or cart-pole engine: an error that names the kind
#define MAZE_REFUSE(h, call)                                                                    \
    do {                                                                                        \
        if ((h)->maze) return (h)->fail("%s is not available on a DNE_KIND_MAZE engine (kind %d): the hard maze has no Atari frames, reference batch, genomes or byte BCs", call, DNE_KIND_MAZE); \
        if ((h)->cartpole) return (h)->fail("%s is not available on a DNE_KIND_CARTPOLE engine (kind %d): the cart-pole has no Atari frames, reference batch, genomes or byte BCs", call, DNE_KIND_CARTPOLE); \
        if ((h)->pendulum) return (h)->fail("%s is not available on a DNE_KIND_PENDULUM engine (kind %d): the pendulum has no Atari frames, reference batch, genomes or byte BCs", call, DNE_KIND_PENDULUM); \
        if ((h)->mjmaze) return (h)->fail("%s is not available on a DNE_KIND_MJMAZE engine (kind %d): MujocoPolicy on the hard maze has no Atari frames, reference batch, genomes or byte BCs", call, DNE_KIND_MJMAZE); \
        if ((h)->dense) return (h)->fail("%s is not available on a DNE_KIND_DENSE engine (kind %d): a dense policy on a step environment has no Atari frames, reference batch, genomes or byte BCs", call, DNE_KIND_DENSE); \
    } while (0)

// ------------------------------------------------------------------------------- env kernels
struct EnvArgs {
    uint8_t *ram_prev, *ram_cur;     // [M][128]
    uint8_t *stacks;                 // [M][84][84][4]
    const ResizeLds *T;
    float *ret, *sign, *step_reward; // [M]
    int32_t *len, *done, *stepped;
    const int32_t *action;
    int32_t *step_counter;           // one counter per launch set: members actually stepped (profiling)
    uint8_t *bc;
    int bc_mode;                     // 0 none, 1 RAM per step (ES, policies.py:410,418), 2 final RAM (GA, policies.py:510)
    int bc_max_steps;
    int immortal;                    // DNE_DEBUG_IMMORTAL (timing experiments only): game over does not end the episode, only tslimit does
    // speculative tail (k_env_spec / k_env_render_spec / k_tail_select): the outcome of EVERY action from the current state,
    // indexed by (position in the active list, action)
    uint8_t *spec_prev, *spec_cur;   // [SPEC_CAP * 32][128] RAM rows before / after the step's last frame
    int32_t *spec_rw;                // [SPEC_CAP * 32][2]: reward, game over
    uint8_t *spec_stacks;            // [SPEC_CAP * 32][84][84][4]
    float *spec_y1;                  // [SPEC_CAP * 32][441][16]: conv1 of every candidate stack (the next step starts at conv2)
    // tail table (forward.h TailTable): position in the window -> member, in the kernel arguments; tt_n = 0: read the list
    int tt_n;
    int tt_member[TT_MAX];
};

__device__ __forceinline__ int env_member(const EnvArgs &E, const int *__restrict__ list, int gsize, int b) {
    if (E.tt_n > 0) return E.tt_member[b];
    const int g = list ? list[b / gsize] : b / gsize;
    return g * gsize + b % gsize;
}

// The emulator state is 40 live bytes per member (RAM bytes 40..127 stay zero).  The per-frame logic is branchy
// scalar code: it runs one member per lane on a register-resident copy of the state (struct Emu); the pixel work
// runs with one or more workgroups per member.
__device__ __forceinline__ Emu ram_load(const uint8_t *row) {
    uint32_t w[RAM_LIVE / 4];
#pragma unroll
    for (int j = 0; j < RAM_LIVE / 4; j++) w[j] = ((const uint32_t *)row)[j];
    return emu_unpack(w);
}
__device__ __forceinline__ void ram_store(const Emu &e, uint8_t *row) {
    uint32_t w[RAM_LIVE / 4];
    emu_pack(e, w);
#pragma unroll
    for (int j = 0; j < RAM_LIVE / 4; j++) ((uint32_t *)row)[j] = w[j];
}

// MaxAndSkipEnv (atari_wrappers.py:88-107): 4 raw frames, rewards summed, early stop on game over;
// prev / cur are the RAM before / after the last executed frame.
#ifdef DNE_PHASE_CLOCK
// Profiling build only (DNE_ENV_BURN): what the headline would do if a raw frame cost what a 6507 + TIA
// interpreter costs -- every lane that steps an emulator spends this many extra lane-instructions per raw frame on a dependent integer
// chain (four per iteration) whose result nobody reads.  The fixture's own frame is ~60; results are unchanged.
__device__ int g_env_burn = 0;
#endif
__device__ inline int skip4(Emu &prev, Emu &cur, int action, int *over) {
    int tot = 0;
    *over = 0;
    for (int i = 0; i < 4; i++) {
        prev = cur;
#ifdef DNE_PHASE_CLOCK
        {
            unsigned x = cur.rng + (unsigned)i;
            for (int b = g_env_burn >> 2; b > 0; b--) {
                x = x * 1664525u + 1013904223u;
                asm volatile("" : "+v"(x));
            }
        }
#endif
        tot += emu_frame(cur, action);
        if (cur.over) { *over = 1; break; }
    }
    return tot;
}

__global__ __launch_bounds__(64) void k_env_reset_logic(EnvArgs E, const uint32_t *__restrict__ seeds, int n) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n) return;
    const uint32_t seed = seeds[m];
    Emu cur = emu_reset(seed), prev = cur;            // env.reset()
    const int noops = 1 + (int)(seed % 30u);         // atari_wrappers.py:18-31 (count fixed by the seed)
    for (int i = 0; i < noops; i++) { prev = cur; emu_frame(cur, 0); }
    int over;
    skip4(prev, cur, 1, &over);                      // atari_wrappers.py:40-48 FIRE then action 2
    skip4(prev, cur, 2, &over);
    uint32_t *gp = (uint32_t *)(E.ram_prev + (size_t)m * 128), *gc = (uint32_t *)(E.ram_cur + (size_t)m * 128);
    for (int j = RAM_LIVE / 4; j < 32; j++) { gp[j] = 0u; gc[j] = 0u; }
    ram_store(prev, (uint8_t *)gp);
    ram_store(cur, (uint8_t *)gc);
    E.ret[m] = 0.0f; E.sign[m] = 0.0f; E.step_reward[m] = 0.0f; E.len[m] = 0; E.done[m] = 0; E.stepped[m] = 1;
}

// the episode bookkeeping of one wrapped step of member m (policies.py:399-425) from its outcome: packed RAM before / after the
// step's last frame, reward, game over.  lds_prev / lds_cur (optional): LDS copies of the RAM rows for a renderer in the same kernel.
struct EnvBook { int t; float ret, sign; };   // a member's step count and return accumulators, read ahead of the commit
__device__ __forceinline__ void env_commit(const EnvArgs &E, int m, const uint32_t (&wp)[RAM_LIVE / 4], const uint32_t (&wc)[RAM_LIVE / 4],
                                           int r, int over, int tslimit, uint8_t *lds_prev = nullptr, uint8_t *lds_cur = nullptr,
                                           const EnvBook *book = nullptr) {
    uint8_t *gp = E.ram_prev + (size_t)m * 128, *gc = E.ram_cur + (size_t)m * 128;
#pragma unroll
    for (int j = 0; j < RAM_LIVE / 4; j++) { ((uint32_t *)gp)[j] = wp[j]; ((uint32_t *)gc)[j] = wc[j]; }
    if (lds_prev) {
#pragma unroll
        for (int j = 0; j < RAM_LIVE / 4; j++) { ((uint32_t *)lds_prev)[j] = wp[j]; ((uint32_t *)lds_cur)[j] = wc[j]; }
    }
    const int t = book ? book->t : E.len[m];
    if (E.bc_mode == 1 && t < E.bc_max_steps) {     // policies.py:410,418 RAM after every step
        uint32_t *d = (uint32_t *)(E.bc + ((size_t)m * E.bc_max_steps + t) * 128);
#pragma unroll
        for (int j = 0; j < RAM_LIVE / 4; j++) d[j] = wc[j];
    }
    if (E.bc_mode == 2) {                           // policies.py:510 final RAM
        uint32_t *d = (uint32_t *)(E.bc + (size_t)m * 128);
#pragma unroll
        for (int j = 0; j < RAM_LIVE / 4; j++) d[j] = wc[j];
    }
    E.ret[m] = (book ? book->ret : E.ret[m]) + (float)r;                               // es.py:425 rews.sum()
    E.sign[m] = (book ? book->sign : E.sign[m]) + (float)((r > 0) - (r < 0));          // es.py:423 np.sign(rews).sum()
    E.step_reward[m] = (float)r;
    E.len[m] = t + 1;
    E.stepped[m] = 1;
    if (E.step_counter) atomicAdd(E.step_counter, 1);
    if ((over && !E.immortal) || t + 1 >= tslimit) E.done[m] = 1;   // policies.py:401,424-425
}

// one wrapped step of member m (atari_wrappers.py:88-107 skip-4) + its bookkeeping; the caller is a single lane
__device__ __forceinline__ void env_member_step(const EnvArgs &E, int m, int action, int tslimit, uint8_t *lds_prev = nullptr,
                                                uint8_t *lds_cur = nullptr) {
    Emu cur = ram_load(E.ram_cur + (size_t)m * 128), prev = cur;   // skip4 overwrites prev before its first use
    int over;
    const int r = skip4(prev, cur, action, &over);
    uint32_t wp[RAM_LIVE / 4], wc[RAM_LIVE / 4];
    emu_pack(prev, wp);
    emu_pack(cur, wc);
    env_commit(E, m, wp, wc, r, over, tslimit, lds_prev, lds_cur);
}

// Speculative tail.  With a handful of members left a lock-step is a latency chain, forward pass -> emulator -> renderer, on a
// nearly idle chip.  The emulator and the renderer do not need the forward pass, only its 1-of-nact answer: while the forward
// pass of step t runs, these two kernels work out the step for EVERY action from the state after step t - 1 (one lane per
// (member, action); a candidate frame stack per action), and k_tail_select only has to adopt the candidate of the action the
// policy picks.  Nothing is predicted and nothing is ever rolled back; the arithmetic per (member, action) is env_member_step's.
constexpr int SPEC_ACTIONS = 32;   // stride of the candidate arrays (>= n_actions)
__global__ __launch_bounds__(64) void k_env_logic(EnvArgs E, const int *__restrict__ list, int gsize, int n_items, int tslimit) {
    DNE_WG_BEGIN;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < n_items) {
        const int m = env_member(E, list, gsize, b);
        if (E.done[m]) E.stepped[m] = 0;
        else env_member_step(E, m, E.action[m], tslimit);
    }
    DNE_WG_END(3);
}

// max over the last two raw frames + WarpFrame + FrameStack for every member stepped by the logic kernel
__device__ __forceinline__ void render_body(EnvLds &s, const EnvArgs &E, int m, bool fill, int band, int nbands) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        s.ram_prev[tid] = E.ram_prev[(size_t)m * 128 + tid];
        s.ram_cur[tid] = E.ram_cur[(size_t)m * 128 + tid];
    }
    __syncthreads();
    synth_observe<1>(s, (uint32_t *)(E.stacks + (size_t)m * OB_BYTES), fill, band, nbands);
}

__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(6, 6))) void k_env_render(EnvArgs E, const int *__restrict__ list, int gsize, int fill, int nbands) {
    __shared__ __attribute__((aligned(16))) EnvLds s;
    const int b = blockIdx.x / nbands, band = blockIdx.x % nbands;
    DNE_PHASE(0, 0);
    DNE_WG_BEGIN;
    const int m = env_member(E, list, gsize, b);
    const int stepped = E.stepped[m];   // asked for first, looked at once the tables are on their way
    synth_load_tables(s, E.T);
    if (!stepped) return;
    render_body(s, E, m, fill != 0, band, nbands);
    DNE_PHASE(0, 4);
    DNE_WG_END(4);
}

// Tail of a generation (a few dozen members left, every kernel boundary is a visible bubble): one workgroup per
// member finishes the policy's forward pass from the fc partial sums (k_out's arithmetic: ((s0+s1)+(s2+s3)) + bias,
// bn3, relu, the 256 x nact output layer as ordered fmaf chains, first-maximum argmax), steps the emulator with the
// chosen action on one lane, and renders the new observation -- k_out + k_env_logic + k_env_render in one launch.
struct RamLds { uint8_t ram_prev[128], ram_cur[128]; };

template <bool RENDER>
struct HeadLds {
    __attribute__((aligned(16))) std::conditional_t<RENDER, EnvLds, RamLds> s;
    float red[4][1][OUT_NA];
    float lg[32];
};

// The policy head + emulator step of one member, by one workgroup (>= 256 threads; the first 256 are the output layer's 256
// inputs: forward.h out_products / out_wave_sums).  Everything that does not depend on the fc partial sums (this thread's
// output-layer weights, the RAM rows, the resize tables) is issued before wait() -- a hook a producer / consumer variant would
// block in; the kernels in use pass NoWait.
template <bool HAS_BN, bool RENDER, bool TT, typename WaitFn>
__device__ __forceinline__ void head_body(HeadLds<RENDER> &H, const FwdArgs &A, const EnvArgs &E, int m, int tslimit,
                                          const float *__restrict__ y3t, float *__restrict__ y3, int32_t *__restrict__ actions,
                                          WaitFn wait, int pos /* position in the window (tail table), or -1 */,
                                          int spec_pos = -1 /* >= 0: adopt the speculated outcome at this list position */) {
    auto &s = H.s;
    float (&lg)[32] = H.lg;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const Layout &L = A.L;
    const int nact = L.nact;
    Item who;
    who.member = m; who.pos = TT ? pos : -1;
    const float sc = item_scale<TT>(A, who);
    const float *base = item_base<TT>(A, who);
    const float *noise_slice = item_eps<TT>(A, who);
    // speculative tail: thread a reads candidate a's outcome (and the member's bookkeeping) now, long before the choice is known
    uint32_t cwp[RAM_LIVE / 4] = {}, cwc[RAM_LIVE / 4] = {};
    int c_r = 0, c_over = 0;
    EnvBook book = {0, 0.0f, 0.0f};
    if (spec_pos >= 0 && tid < nact) {
        const size_t c = (size_t)spec_pos * SPEC_ACTIONS + tid;
#pragma unroll
        for (int j = 0; j < RAM_LIVE / 4; j++) {
            cwp[j] = ((const uint32_t *)(E.spec_prev + c * 128))[j];
            cwc[j] = ((const uint32_t *)(E.spec_cur + c * 128))[j];
        }
        c_r = E.spec_rw[2 * c]; c_over = E.spec_rw[2 * c + 1];
        book.t = E.len[m]; book.ret = E.ret[m]; book.sign = E.sign[m];
    }
    if (spec_pos < 0 && tid < 64) {
        s.ram_prev[tid] = E.ram_prev[(size_t)m * 128 + tid];
        s.ram_cur[tid] = E.ram_cur[(size_t)m * 128 + tid];
    }
    // a workgroup with more than the output layer's four waves steps the emulator for EVERY action on the lanes of its fifth wave
    // while the others wait for their weights: the emulator does not need the forward pass, only its 1-of-nact answer (the
    // speculative tail's idea inside one launch).  The lane of the chosen action commits; nothing is predicted or rolled back.
    const bool own_candidates = spec_pos < 0 && blockDim.x > 256;
    if (own_candidates && tid >= 256 && tid < 256 + nact) {
        Emu cur = ram_load(E.ram_cur + (size_t)m * 128), prev = cur;   // skip4 overwrites prev before its first use
        c_r = skip4(prev, cur, tid - 256, &c_over);
        emu_pack(prev, cwp);
        emu_pack(cur, cwc);
        book.t = E.len[m]; book.ret = E.ret[m]; book.sign = E.sign[m];
    }
    // this thread's row of the output layer (k = tid): nact consecutive weights of the base vector and of the noise slice
    float wth[OUT_NA], wep[OUT_NA];
    float fbt = 0.0f, fbe = 0.0f, s3 = 1.0f, h3 = 0.0f;
    if (tid < 256) {
        const float *wb = base + L.ow + tid * nact, *we = noise_slice + L.ow + tid * nact;
#pragma unroll
        for (int a = 0; a < OUT_NA; a++) {
            wth[a] = a < nact ? wb[a] : 0.0f;
            wep[a] = a < nact ? we[a] : 0.0f;
        }
        fbt = opt_bias(L.fcb, base[opt_off(L.fcb) + tid]); fbe = opt_bias(L.fcb, noise_slice[opt_off(L.fcb) + tid]);
        if (HAS_BN) { s3 = A.bn[(size_t)m * 608 + 96 + tid]; h3 = A.bn[(size_t)m * 608 + 352 + tid]; }
    }
    if constexpr (RENDER) synth_load_tables(s, E.T);
    if (!wait()) return;
    DNE_PHASE(3, 1);
    if (tid < 256) {
        float t = fc_combine(y3t, m, tid, A.sub_sums != 0);
        float pvb = sc * fbe;
        const float fb = fbt + pvb;
        t = t + fb;
        y3[(size_t)m * 256 + tid] = t;
        if (HAS_BN) {
            t = t * s3;
            t = t + h3;
        }
        const float x = t > 0.0f ? t : 0.0f;
        float pr[1][OUT_NA];
#pragma unroll
        for (int a = 0; a < OUT_NA; a++) {
            float pv = sc * wep[a];
            float w = wth[a] + pv;
            pr[0][a] = x * w;
        }
        out_wave_sums<1>(pr, nact, H.red[wv], lane);
    }
    __syncthreads();
    DNE_PHASE(3, 2);
    if (tid < nact) {
        const float s01 = H.red[0][0][tid] + H.red[1][0][tid];
        const float s23 = H.red[2][0][tid] + H.red[3][0][tid];
        const float t = s01 + s23;
        float pv = sc * noise_slice[L.ob + tid];
        const float bias = base[L.ob + tid] + pv;
        lg[tid] = t + bias;
    }
    __syncthreads();
    DNE_PHASE(3, 3);
    if (spec_pos >= 0) {   // the emulator + renderer outcome of every action is on the table: every thread finds the policy's
        int best = 0;      // choice, the thread that read that candidate commits it, all copy its frame stack
        for (int a = 1; a < nact; a++)
            if (lg[a] > lg[best]) best = a;   // tf.argmax: first maximum
        if (tid == best) {
            actions[m] = best;
            env_commit(E, m, cwp, cwc, c_r, c_over, tslimit, nullptr, nullptr, &book);
        }
        const uint4 *src = (const uint4 *)(E.spec_stacks + ((size_t)spec_pos * SPEC_ACTIONS + best) * OB_BYTES);
        uint4 *dst = (uint4 *)(E.stacks + (size_t)m * OB_BYTES);
        for (int i0 = tid; i0 < OB_BYTES / 16; i0 += 8 * blockDim.x) {   // all of a thread's loads in flight before its first store
            uint4 v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) { const int i = i0 + j * blockDim.x; if (i < OB_BYTES / 16) v[j] = src[i]; }
#pragma unroll
            for (int j = 0; j < 8; j++) { const int i = i0 + j * blockDim.x; if (i < OB_BYTES / 16) dst[i] = v[j]; }
        }
        return;
    }
    if (own_candidates) {
        int best = 0;
        for (int a = 1; a < nact; a++)
            if (lg[a] > lg[best]) best = a;   // tf.argmax: first maximum
        if (tid == 256 + best) {
            actions[m] = best;
            env_commit(E, m, cwp, cwc, c_r, c_over, tslimit, RENDER ? s.ram_prev : nullptr, RENDER ? s.ram_cur : nullptr, &book);
        }
    } else if (tid == 0) {
        int best = 0;
        for (int a = 1; a < nact; a++)
            if (lg[a] > lg[best]) best = a;   // tf.argmax: first maximum
        actions[m] = best;
        env_member_step(E, m, best, tslimit, RENDER ? s.ram_prev : nullptr, RENDER ? s.ram_cur : nullptr);
    }
    if constexpr (RENDER) {
        __syncthreads();
        synth_observe(s, (uint32_t *)(E.stacks + (size_t)m * OB_BYTES), false);
    }
}

template <bool HAS_BN, bool RENDER>
__global__ __launch_bounds__(1024) void k_tail_step(FwdArgs A, EnvArgs E, const int *__restrict__ list, int gsize, int tslimit,
                                                     const float *__restrict__ y3t, float *__restrict__ y3,
                                                     int32_t *__restrict__ actions) {
    __shared__ HeadLds<RENDER> H;
    const int b = blockIdx.x;
    DNE_PHASE(3, 0);
    const int m = env_member(E, list, gsize, b);
    if (E.done[m]) { if (threadIdx.x == 0) E.stepped[m] = 0; return; }
    if (A.tt.n > 0) head_body<HAS_BN, RENDER, true>(H, A, E, m, tslimit, y3t, y3, actions, NoWait{}, b);
    else head_body<HAS_BN, RENDER, false>(H, A, E, m, tslimit, y3t, y3, actions, NoWait{}, b);
#ifdef DNE_PHASE_CLOCK
    __syncthreads();
    DNE_PHASE(3, 4);
#endif
}

// The two speculative kernels ride in launches of the forward pass (same stream, no event traffic -- a cross-stream event
// hand-over per lock-step costs more than the lock-step): the emulator lanes share conv1's launch, the candidate renderers share
// the quad fc's (they need the emulator's output, i.e. a kernel boundary, and the fc is the longest stage to hide under).
__global__ __launch_bounds__(256) void k_conv1_spec(FwdArgs A, EnvArgs E, const int *__restrict__ list, int gsize,
                                                    float *__restrict__ y1, int nsplit, int n_conv_blocks, int n_items, int nact) {
    __shared__ Conv1Lds S;
    if ((int)blockIdx.x < n_conv_blocks) {
        if (A.tt.n > 0) {
            const Item it = decode_item<true>(A, blockIdx.x / nsplit, list, gsize, 1, 0, E.stacks, nullptr, A.done);
            if (it.skip) return;
            conv1_body<16, true>(S, A, it, y1, blockIdx.x % nsplit, nsplit);
        } else {
            const Item it = decode_item(A, blockIdx.x / nsplit, list, gsize, 1, 0, E.stacks, nullptr, A.done);
            if (it.skip) return;
            conv1_body(S, A, it, y1, blockIdx.x % nsplit, nsplit);
        }
        return;
    }
    const int i = ((int)blockIdx.x - n_conv_blocks) * 256 + threadIdx.x;
    if (i >= n_items * nact) return;
    const int b = i / nact, a = i % nact;
    const int m = env_member(E, list, gsize, b);
    if (E.done[m]) return;
    Emu cur = ram_load(E.ram_cur + (size_t)m * 128), prev = cur;
    int over;
    const int r = skip4(prev, cur, a, &over);
    const size_t c = (size_t)b * SPEC_ACTIONS + a;
    ram_store(prev, E.spec_prev + c * 128);
    ram_store(cur, E.spec_cur + c * 128);
    E.spec_rw[2 * c] = r;
    E.spec_rw[2 * c + 1] = over;
}

// conv2 of the forward pass + the emulator outcome of every action.  y1_cand: the member's conv1 output is the candidate its
// last action selected (k_tail_select_conv1 of the previous lock-step), not a row of y1.
template <bool HAS_BN>
__global__ __launch_bounds__(256) void k_conv2_spec(FwdArgs A, EnvArgs E, const int *__restrict__ list, int gsize,
                                                    const float *__restrict__ y1, float *__restrict__ y2, int nsplit, int n_conv_blocks,
                                                    int n_items, int nact, const int32_t *__restrict__ last_action) {
    __shared__ Conv2Lds S;
    if ((int)blockIdx.x < n_conv_blocks) {
        const int b = blockIdx.x / nsplit;
        if (A.tt.n > 0) {
            const Item it = decode_item<true>(A, b, list, gsize, 1, 0, nullptr, nullptr, A.done);
            if (it.skip) return;
            const float *row = E.spec_y1 + ((size_t)b * SPEC_ACTIONS + last_action[it.member]) * 7056;
            conv2_body<HAS_BN, true>(S, A, it, y1, y2, blockIdx.x % nsplit, nsplit, nullptr, row);
        } else {
            const Item it = decode_item(A, b, list, gsize, 1, 0, nullptr, nullptr, A.done);
            if (it.skip) return;
            const float *row = E.spec_y1 + ((size_t)b * SPEC_ACTIONS + last_action[it.member]) * 7056;
            conv2_body<HAS_BN>(S, A, it, y1, y2, blockIdx.x % nsplit, nsplit, nullptr, row);
        }
        return;
    }
    const int i = ((int)blockIdx.x - n_conv_blocks) * 256 + threadIdx.x;
    if (i >= n_items * nact) return;
    const int b = i / nact, a = i % nact;
    const int m = env_member(E, list, gsize, b);
    if (E.done[m]) return;
    Emu cur = ram_load(E.ram_cur + (size_t)m * 128), prev = cur;
    int over;
    const int r = skip4(prev, cur, a, &over);
    const size_t c = (size_t)b * SPEC_ACTIONS + a;
    ram_store(prev, E.spec_prev + c * 128);
    ram_store(cur, E.spec_cur + c * 128);
    E.spec_rw[2 * c] = r;
    E.spec_rw[2 * c + 1] = over;
}

template <int NV, bool HAS_BN>
__global__ __launch_bounds__(256) void k_fc_quad_spec(FwdArgs A, EnvArgs E, const int *__restrict__ list, int gsize,
                                                      const float *__restrict__ y2, float *__restrict__ y3t, int n_fc_blocks,
                                                      int nact, int nbands) {
    constexpr size_t LDS_BYTES = sizeof(EnvLds) > sizeof(QuadLds<NV>) ? sizeof(EnvLds) : sizeof(QuadLds<NV>);
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    if ((int)blockIdx.x < n_fc_blocks) {
        QuadLds<NV> &S = *reinterpret_cast<QuadLds<NV> *>(lds);
        const int item = blockIdx.x >> 6, cg = (blockIdx.x >> 2) & 15, sl = blockIdx.x & 3;
        if (A.tt.n > 0) fc_quad_body<NV, HAS_BN, true>(S, A, list, item, cg, sl, y2, y3t);
        else fc_quad_body<NV, HAS_BN, false>(S, A, list, item, cg, sl, y2, y3t);
        return;
    }
    EnvLds &s = *reinterpret_cast<EnvLds *>(lds);
    const int rb = (int)blockIdx.x - n_fc_blocks;
    const int band = rb % nbands, ba = rb / nbands, b = ba / nact, a = ba % nact;
    const int m = env_member(E, list, gsize, b);
    if (E.done[m]) return;
    synth_load_tables(s, E.T);
    const size_t c = (size_t)b * SPEC_ACTIONS + a;
    const int tid = threadIdx.x;
    if (tid < 64) {
        s.ram_prev[tid] = E.spec_prev[c * 128 + tid];
        s.ram_cur[tid] = E.spec_cur[c * 128 + tid];
    }
    __syncthreads();
    synth_observe(s, (uint32_t *)(E.spec_stacks + c * OB_BYTES), false, band, nbands, (const uint32_t *)(E.stacks + (size_t)m * OB_BYTES));
}

template <bool HAS_BN>
__global__ __launch_bounds__(1024) void k_tail_select(FwdArgs A, EnvArgs E, const int *__restrict__ list, int gsize, int tslimit,
                                                       const float *__restrict__ y3t, float *__restrict__ y3,
                                                       int32_t *__restrict__ actions) {
    __shared__ HeadLds<false> H;
    const int b = blockIdx.x;
    const int m = env_member(E, list, gsize, b);
    if (E.done[m]) { if (threadIdx.x == 0) E.stepped[m] = 0; return; }
    if (A.tt.n > 0) head_body<HAS_BN, false, true>(H, A, E, m, tslimit, y3t, y3, actions, NoWait{}, b, b);
    else head_body<HAS_BN, false, false>(H, A, E, m, tslimit, y3t, y3, actions, NoWait{}, b, b);
}

// k_tail_select + conv1 of every candidate frame stack (workgroups past the first n_items): whichever action the policy picks in
// the same launch, the next lock-step finds its conv1 output ready and starts at conv2.
template <bool HAS_BN>
__global__ __launch_bounds__(256) void k_tail_select_conv1(FwdArgs A, EnvArgs E, const int *__restrict__ list, int gsize, int tslimit,
                                                           const float *__restrict__ y3t, float *__restrict__ y3,
                                                           int32_t *__restrict__ actions, int n_items, int nact, int nsplit) {
    constexpr size_t LDS_BYTES = sizeof(HeadLds<false>) > sizeof(Conv1Lds) ? sizeof(HeadLds<false>) : sizeof(Conv1Lds);
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    if ((int)blockIdx.x < n_items) {
        HeadLds<false> &H = *reinterpret_cast<HeadLds<false> *>(lds);
        const int b = blockIdx.x;
        const int m = env_member(E, list, gsize, b);
        if (E.done[m]) { if (threadIdx.x == 0) E.stepped[m] = 0; return; }
        if (A.tt.n > 0) head_body<HAS_BN, false, true>(H, A, E, m, tslimit, y3t, y3, actions, NoWait{}, b, b);
        else head_body<HAS_BN, false, false>(H, A, E, m, tslimit, y3t, y3, actions, NoWait{}, b, b);
        return;
    }
    Conv1Lds &S = *reinterpret_cast<Conv1Lds *>(lds);
    const int cb = (int)blockIdx.x - n_items, part = cb % nsplit, ba = cb / nsplit, b = ba / nact, a = ba % nact;
    Item it;
    it.member = env_member(E, list, gsize, b);
    it.pos = A.tt.n > 0 ? b : -1;
    if (E.done[it.member]) return;
    it.row = b * SPEC_ACTIONS + a;
    it.ob = E.spec_stacks + (size_t)it.row * OB_BYTES;
    it.skip = false;
    if (A.tt.n > 0) conv1_body<16, true>(S, A, it, E.spec_y1, part, nsplit);
    else conv1_body(S, A, it, E.spec_y1, part, nsplit);
}

// order-preserving compaction of the active-group list
__global__ __launch_bounds__(1024) void k_compact(const int32_t *__restrict__ done, int gsize, const int *__restrict__ list_in,
                                                  int n_in, int *__restrict__ list_out, int *__restrict__ count_out) {
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    int running = 0;
    for (int start = 0; start < n_in; start += 1024) {
        const int i = start + tid;
        int g = -1;
        bool alive = false;
        if (i < n_in) {
            g = list_in ? list_in[i] : i;
            for (int k = 0; k < gsize; k++) alive = alive || !done[g * gsize + k];
        }
        const unsigned long long bal = __ballot(alive);
        if (lane == 0) wave_tot[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < 16; k++) { before += k < wv ? wave_tot[k] : 0; total += wave_tot[k]; }
        if (alive) {
            const int pos = running + before + __popcll(bal & ((1ull << lane) - 1ull));
            list_out[pos] = g;
            if (pos < TT_MAX) count_out[8 + pos] = g;   // the head of the list travels to the host with the count (tail table)
        }
        running += total;
        __syncthreads();
    }
    if (tid == 0) *count_out = running;
}

__global__ void k_iota(int *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}

// ------------------------------------------------------------------------------- launch plan
// plan.h decides what a lock-step launches (Knobs + PlanFacts + the active count -> StepPlan per burst -> WindowPlan per window); the launchers
// below take those values as arguments.  The empty StepPlan is what every caller outside an evaluation passes (dne_act).
constexpr int N_STREAMS = 4;   // the main stream + 3 window streams: more than four windows measured slower (round 3, 5 / 6 / 8 at full width: +7.5 / +5.4 / +7.2 %; round 4 with one k_fc_duo workgroup per CU: +8.4 / +5.9 / +4.4 %)

// the members of a tail table as arguments of the emulator's kernels (null: no table in force)
static void set_tail_table(EnvArgs &E, const TailTable *tt) {
    E.tt_n = tt ? tt->n : 0;
    if (tt) memcpy(E.tt_member, tt->member, sizeof(E.tt_member));
}

// a run-time bool as a template argument: f(std::true_type{}) or f(std::false_type{}), so that a launch is written once
template <class F> static inline void with_bool(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <int V> using int_c = std::integral_constant<int, V>;

// the default reference route (k_conv1_ref_shared<16>, k_conv2_ref<16, true>, the matrix-core fc): the one the dedup route may replace
static bool ref_default_route(const Knobs &k, int F) { return k.conv1_shared && k.conv1_fpw >= 8 && (F == 16 || F == 32 || F == 64 || F == 128); }

// ------------------------------------------------------------------------------- handle
struct dne_handle {
    dne_config cfg{};
    Layout L{};
    std::string err;
    hipStream_t stream = nullptr;
    std::vector<hipStream_t> sub_streams;   // sub-batch streams (sub_streams[0] == stream)
    Knobs k;                         // the DNE_* scheduling and tuning knobs (plan.h: one table), read once by dne_create
    double dense_scale = 1.0;        // table length / the stretch of the table this evaluation's noise slices cover (dne_es_eval; 1 for every other caller): a rank that draws
                                     // its indices from its own 1/N of the table (es.py shard 'table') holds pairs as dense as N times as many over the whole table
    float *noise_pre = nullptr;      // the noise table scaled by the evaluation's sigma, fl(sigma * eps) entry by entry (k_scale_table): k_fc_ring<true>'s DMA source.  Built the first
                                     // time an evaluation enters the ring's range at that sigma (ES runs keep one sigma: once per run, 0.4 ms), dropped with the table
    size_t noise_pre_count = 0;      // entries of the table the copy was made from (0: none)
    float noise_pre_sigma = 0.0f;    // the sigma it holds
    bool noise_pre_no_room = false;  // the copy did not fit once: the ring scales its rows itself from then on
    bool pair_sigma_uniform = false; // every pair of the member set is (+s, -s) with ONE s (dne_set_members)
    float pair_sigma = 0.0f;
    float *theta_perm = nullptr;     // [3872 + 16][256]: base slot 0's fc matrix, every row stored as columns l, l+64, l+128, l+192 per lane (k_theta_perm, once per evaluation)
    float *y3s = nullptr;            // [member][32][256]: the chain sums k_fc_sub leaves for k_out<.., SUB>
    int *unit_order = nullptr;       // [4 * groups]: per window, its (group, k-slice) units in noise-table order
    float *zero_rows = nullptr;      // [ZERO_ROWS_FLOATS] zeros: what k_fc_sub fetches in place of a dead weight row (FwdArgs::zero_rows)
    uint8_t *spec_prev = nullptr, *spec_cur = nullptr, *spec_stacks = nullptr;   // candidate outcomes of the speculative tail (DNE_SPEC_MAX)
    int32_t *spec_rw = nullptr;
    float *spec_y1 = nullptr;
    bool uniform_base = false;       // every member perturbs the same base slot (dne_set_members checks)
    bool antithetic_slot0 = false;   // what k_theta_perm + k_fc_ring assume, checked member by member in dne_set_members: base slot 0 everywhere and
                                     // members (2i, 2i+1) = (offset, +s), (the same offset, -s) -- es.py:412-419's pairs, nothing else
    int M = 0, F = 0, ref_chunk = 0;
    size_t base_stride = 0;
    // device memory
    float *noise = nullptr; size_t noise_count = 0;
    float *bases = nullptr; int base_cap = 0;
    float *opt_m = nullptr, *opt_v = nullptr, *g = nullptr; int opt_t = 0;
    double *partial = nullptr;
    uint8_t *ref = nullptr; bool ref_set = false;
    float *ref_f32 = nullptr;        // the reference frames as padded planar floats (k_conv1_ref_shared)
    // the reference batch as unique convolution operands (ref_index.h), uploaded by dne_set_ref_batch when the engine's knobs take the
    // default reference route; ref_dedup says whether this batch has few enough distinct rows for that route to pay
    float *ref_tab1 = nullptr;       // [ref_cap1][256]: the unique conv1 patches as floats, k = (kh, kw, c); rows past U1 are zeros
    int32_t *ref_idx1 = nullptr;     // [F][448]: patch id per conv1 position (positions past 441: id 0, never counted)
    int32_t *ref_win = nullptr;      // [ref_cap2][16]: the unique conv2 windows as patch ids, -1 = SAME padding; rows past U2 are all -1
    int32_t *ref_idx2 = nullptr;     // [F][128]: window id per conv2 position (positions past 120 repeat position 120)
    int ref_cap1 = 0, ref_cap2 = 0;  // rows the two tables can hold (0: the knobs name another route)
    int ref_U1 = 0, ref_U2 = 0, ref_U1p = 0, ref_U2p = 0;
    bool ref_dedup = false;
    int32_t *m_slot = nullptr; int64_t *m_off = nullptr; float *m_scale = nullptr;
    std::vector<int32_t> host_slot; std::vector<int64_t> host_off; std::vector<float> host_scale;   // what dne_set_members uploaded
    std::vector<int32_t> host_caller;   // the caller's index of each of those members (dne_ga_eval* reorders them; otherwise the identity)
    float *bn = nullptr, *bn_mom = nullptr;
    uint8_t *ram_prev = nullptr, *ram_cur = nullptr, *stacks = nullptr;
    ResizeLds *tables = nullptr;
    float *ret = nullptr, *sign = nullptr, *step_reward = nullptr, *logits = nullptr;
    int32_t *len = nullptr, *done = nullptr, *action = nullptr, *stepped = nullptr;
    int32_t *launch_units = nullptr; size_t launch_units_cap = 0;
    uint32_t *seeds = nullptr;
    float *y1 = nullptr, *y2 = nullptr, *y3 = nullptr, *y3t = nullptr;   // step mode: one row per member (y3t: 4 k-slice partials)
    bool members_materialized = false;   // the current members are plain vectors (scale 0 everywhere): kernels that have one skip the noise stream
    std::vector<int> child_slots;    // base slots set aside for materialised children
    bool maze = false;               // DNE_KIND_MAZE: whole episodes in k_maze_rollout (csrc/maze.h); none of the Atari buffers exist
    maze::Header maze_hdr{}; float *maze_walls = nullptr; int maze_nw = 0;   // dne_maze_set_walls
    float *maze_xy = nullptr; int maze_last_n = 0;   // final (x, y) per member of the last evaluation, and how many members that was
    // novelty on the maze (csrc/maze_novelty.h): the archive of (x, y) points in insertion order, host members' points, the n results
    float *mzn_arch = nullptr; size_t mzn_arch_cap = 0; int mzn_arch_n = 0;
    float *mzn_xy = nullptr; size_t mzn_xy_cap = 0;
    double *mzn_out = nullptr; size_t mzn_out_cap = 0;
    int32_t *mzn_idx = nullptr; size_t mzn_idx_cap = 0;   // member indices of dne_maze_archive_append_members
    double mzn_last_ms = -1.0;
    // Deep-GA on the maze (csrc/maze_ga.h): 3 M slots of base_stride floats apart from `bases` -- the parents' bank as a double buffer
    // (halves of M slots, mzg_half the live one, mzg_T parents in it), then one scratch slot per member for an evaluation's roots -- and
    // the member descriptors of dne_maze_ga_eval / dne_maze_ga_promote, apart from dne_set_members' own.  A DNE_KIND_DENSE handle keeps the
    // same fields for dne_dense_ga_* (csrc/dense_ga.h: the bank with P at run time; a handle is of one kind)
    float *mzg_mem = nullptr; int mzg_half = 0, mzg_T = 0;
    int32_t *mzg_slot = nullptr; int64_t *mzg_off = nullptr; float *mzg_scale = nullptr;
    int32_t *mzg_chain_offs = nullptr; int64_t *mzg_seeds = nullptr; float *mzg_powers = nullptr; size_t mzg_chain_cap = 0;
    std::vector<int32_t> mzg_host_slot; std::vector<float> mzg_host_scale;   // what dne_maze_ga_eval uploaded
    bool cartpole = false;           // DNE_KIND_CARTPOLE: whole episodes in k_cartpole_rollout (csrc/cartpole.h); the maze's create path without walls
    double *cp_state = nullptr; int cp_last_n = 0;   // final (x, x_dot, theta, theta_dot) per member of the last evaluation, and how many members that was
    bool pendulum = false;           // DNE_KIND_PENDULUM: MujocoPolicy on the pendulum swing-up, whole episodes in k_pendulum_rollout (csrc/pendulum.h)
    pendulum::Options pd_opt{};      // outputs, action mode, ob_mean / ob_std, noise std
    double *pd_state = nullptr;      // final (theta, theta_dot) per member of the last evaluation
    // what the two MujocoPolicy kinds (DNE_KIND_PENDULUM, DNE_KIND_MJMAZE: a handle is one of them) keep alike; their Options differ in width
    int pd_hidden = 0, pd_nl = 0;    // hidden width (64 / 128 / 256) and nonlinearity of the engine's policy
    int pd_last_n = 0;               // members of the last evaluation
    struct MujocoOptions {
        bool stat_set = false;       // dne_*_set_ob_stat was called (before it ob_mean / ob_std are NaN and an evaluation is refused)
        double *sum = nullptr, *sumsq = nullptr; int32_t *count = nullptr;   // observation statistics per member of the last evaluation
        int64_t *off = nullptr; uint8_t *flag = nullptr;   // dne_*_set_rollout_options: per member, for the next evaluation only
        int n = 0; bool has_off = false, has_flag = false; std::vector<int64_t> host_off;   // (the offsets once more on the host: checked again at the launch)
    } mo;
    // the step-at-a-time environment batch (csrc/step_env.h, dne_stepenv_*): max_members environments apart from everything an evaluation reads
    // or writes, allocated by the first dne_stepenv_* call that needs it.  se_io_*: what one call uploads and fetches, [max_members] each
    stepenv::Batch se{}; bool se_ready = false; std::vector<uint8_t> se_was_reset;   // (the bitmap: on the host, one byte per environment)
    int32_t *se_io_idx = nullptr, *se_io_steps = nullptr; uint32_t *se_io_seeds = nullptr; float *se_io_act = nullptr, *se_io_rew = nullptr, *se_io_obs = nullptr;
    uint8_t *se_io_done = nullptr; double *se_io_state = nullptr;
    hipEvent_t se_ev_a = nullptr, se_ev_b = nullptr; double se_last_ms = -1.0;   // the last step kernel between two device events
    // DNE_KIND_MJMAZE: MujocoPolicy on the hard maze, whole episodes in k_mjmaze_rollout (csrc/mjmaze.h).  It shares the maze's walls, final
    // positions and archive (maze_*, mzn_*); mj_opt holds its own 11 means and deviations
    bool mjmaze = false;
    mjmaze::Options mj_opt{};
    // Deep-GA on the two MujocoPolicy kinds (csrc/mujoco_ga.h, dne_mujoco_ga_*): the bank is mzg_mem as two halves of mjg_Tmax slots, then
    // mjg_root_cap scratch slots for an evaluation's roots (none until an evaluation has a root); mzg_slot / mzg_off / mzg_scale hold the
    // descriptors; mjg_sc [entry][mjg_sc_stride] the column scales of every entry with a root, mjg_root_idx [entry] its noise index (< 0: none)
    int mjg_Tmax = 0, mjg_sc_stride = 0; size_t mjg_root_cap = 0, mjg_entries = 0;
    float *mjg_sc = nullptr; int64_t *mjg_root_idx = nullptr; std::vector<int64_t> mjg_host_root;
    mujoco_ga::Layout mjg_L{};
    // DNE_KIND_DENSE: a dense policy of the shape dn_shape on the step environment dn_shape.env, k_dense_run (csrc/dense.h)
    bool dense = false;
    dense::Shape dn_shape{};
    double *dn_state = nullptr; int dn_last_n = 0;   // final state records [member][S] of the last evaluation, and how many members that was
    float *dn_bc = nullptr; bool dn_bc_valid = false;   // the BCs [member][D] of the last evaluation (csrc/dense_novelty.h), formed by the first call that needs them
    int32_t *se_io_mem = nullptr; float *se_io_out = nullptr;   // dne_stepenv_act / _run: the member of each listed environment; the raw outputs
    bool episodic() const { return maze || cartpole || pendulum || mjmaze || dense; }   // a whole episode per member in one launch: what dne_es_eval and the record calls accept beside the Atari kinds
    bool large = false;              // DNE_KIND_GA_LARGE: y1 [441][32], y2 / y3 [121][64] (conv3 output), y3t = the 512 fc outputs
    float *y1r[2] = {nullptr, nullptr}, *y2r[2] = {nullptr, nullptr}, *y3pr[2] = {nullptr, nullptr};   // reference pass scratch, two ways
    float *fr1[2] = {nullptr, nullptr}, *fr2[2] = {nullptr, nullptr};   // per-frame batch-norm moments of conv1 / conv2 ([rows][2][C])
    hipEvent_t ev_ref[2] = {nullptr, nullptr};
    int *list_a = nullptr, *list_b = nullptr, *count_dev = nullptr;
    int *count_host = nullptr;       // pinned: the active count comes back once per burst (a pageable destination makes the copy a staged, synchronous one)
    uint8_t *bc = nullptr; size_t bc_bytes = 0;
    float *mat_out = nullptr; size_t mat_cap = 0;
    float *scratch_f = nullptr; size_t scratch_cap = 0;   // small float scratch (ranks, weights)
    int64_t *scratch_i = nullptr;
    // profiling
    std::vector<hipEvent_t> ev_pool;
    std::vector<hipEvent_t> fc_ring;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    dne_profile prof{};
    // GA parent cache: prefix chain -> base slot
    std::map<std::vector<int64_t>, int> ga_cache;
    int ga_cache_mode = 0; float ga_cache_sigma = 0.0f;   // what the cached parents were built with (1 sigma / 2 per-seed powers)
    std::vector<int> free_slots;
    // every device allocation of the handle, each between two poisoned red zones (dne_check_redzones)
    struct Block { std::string name; uint8_t *raw; size_t bytes; };
    std::vector<Block> blocks;
    size_t redzone = 4096;           // bytes on each side (DNE_REDZONE=0 disables)
    bool trace_on = false;           // DNE_TRACE=1: stage breadcrumbs on stderr
    bool staged_copies = true;       // DNE_STAGED_COPY=0: hand large host buffers straight to hipMemcpy (diagnosis only)
    bool debug_sync = false;         // DNE_DEBUG_SYNC=1: synchronize + check after every launch set of an evaluation
    // pinned staging for large host <-> device transfers (the runtime would otherwise pin the caller's pages)
    uint8_t *stage_buf[2] = {nullptr, nullptr};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    // gathered per-pair records of one generation, device-resident (dne_allgather_results / dne_records_set)
    int64_t *rec_idx = nullptr; float *rec_ret = nullptr, *rec_sign = nullptr; int32_t *rec_len = nullptr;
    uint8_t *rec_send = nullptr, *rec_recv = nullptr; size_t rec_cap = 0, rec_wire_cap = 0; int rec_n = 0;
    std::vector<int64_t> rec_idx_host;
    int64_t *chain_offs = nullptr; float *chain_pw = nullptr; size_t chain_cap = 0;   // GA: seed offsets (+ per-seed powers) of the chain being rebuilt
    float *init_scale = nullptr;     // GA genomes in the gpu tree's form: root = noise[idx0] * init_scale (dne_ga_set_init_scale)
    // novelty archive resident on the device (dne_archive_append): rows of all entries back to back
    uint8_t *arch = nullptr; size_t arch_cap = 0, arch_rows = 0; int arch_dim = 0;
    int64_t *arch_row0 = nullptr; int32_t *arch_len = nullptr; size_t arch_ent_cap = 0;
    std::vector<int64_t> arch_row0_host; std::vector<int32_t> arch_len_host;
    size_t arch_pitch = 0;           // bytes per archive row on the device: the width rounded up to 16, zero-padded (novelty.h)
    // dne_novelty_knn scratch: the [n][narch] distances + n results, the length-ordered index arrays, host members' rows
    double *nov_dist = nullptr; size_t nov_dist_cap = 0;
    uint8_t *nov_idx = nullptr; size_t nov_idx_cap = 0;
    uint8_t *nov_rows = nullptr; size_t nov_rows_cap = 0;
    unsigned long long *nov_acc = nullptr; size_t nov_acc_cap = 0;   // [n][narch][2] sums of a row-split distance launch
    // pool novelty over final RAM states (csrc/ram_novelty.h): how many members the last evaluation left one 128-byte row each in bc (0: none
    // yet, or bc holds full trajectories), the caller's index of each row (dne_ga_eval* reorders its members), and the calls' device scratch
    int ram_last_n = 0; std::vector<int32_t> ram_last_caller;
    uint8_t *ram_pts = nullptr; size_t ram_pts_cap = 0;      // a host bc's rows, or the recorded rows in the caller's order
    double *ram_out = nullptr; size_t ram_out_cap = 0;
    int32_t *ram_nb = nullptr; size_t ram_nb_cap = 0;        // [n][kk] neighbours
    int32_t *ram_idx = nullptr; size_t ram_idx_cap = 0;      // bc rows to gather
    double ram_last_ms = -1.0;
    // RCCL communicator (dne_comm_init); the library is opened on demand
    void *rccl_lib = nullptr; void *comm = nullptr; int comm_rank = 0, comm_size = 1;
    bool comm_borrowed = false;      // dne_comm_share: the communicator belongs to another handle of this process
    std::mutex comm_mu;                  // dne_comm_init publishes its communicator and dne_comm_abort retires one under this lock
    std::atomic<bool> comm_off{false};   // dne_comm_abort (possibly from another host thread than a dne_comm_init still in flight): this handle takes no part in RCCL any more, a late result is dropped
    double *comm_scratch = nullptr;

    template <typename T>
    hipError_t alloc(T **p, size_t n, const char *name) {
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T), rz = redzone;
        uint8_t *raw = nullptr;
        hipError_t e = hipMalloc((void **)&raw, bytes + 2 * rz);
        if (e != hipSuccess) { *p = nullptr; return e; }
        if (rz) {
            e = hipMemset(raw, 0xA5, rz);
            if (e == hipSuccess) e = hipMemset(raw + rz + bytes, 0xA5, rz);
            if (e != hipSuccess) { hipFree(raw); *p = nullptr; return e; }
        }
        blocks.push_back({name, raw, bytes});
        *p = (T *)(raw + rz);
        return hipSuccess;
    }
    template <typename T>
    hipError_t release(T *&p) {
        if (!p) return hipSuccess;
        uint8_t *raw = (uint8_t *)p - redzone;
        for (size_t i = 0; i < blocks.size(); i++)
            if (blocks[i].raw == raw) { blocks.erase(blocks.begin() + i); break; }
        p = nullptr;
        return hipFree(raw);
    }
    void trace(const char *fmt, ...) {
        if (!trace_on) return;
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        fprintf(stderr, "[dne %d] %s\n", cfg.device_id, buf);
        fflush(stderr);
    }

    int fail(const char *fmt, ...) {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        err = buf;
        return -1;
    }
    FwdArgs fwd(bool use_done, const StepPlan &p = {}, const TailTable *tt = nullptr) const {
        FwdArgs A;
        A.noise = noise; A.bases = bases; A.base_stride = base_stride;
        A.m_slot = m_slot; A.m_off = m_off; A.m_scale = m_scale; A.bn = bn; A.bn_mom = bn_mom;
        A.done = use_done ? done : nullptr; A.L = L;
        A.zero_rows = zero_rows;
        A.sub_sums = p.sub ? 1 : 0;
        if (tt) A.tt = *tt; else A.tt.n = 0;
        return A;
    }
    EnvArgs env(int bc_mode, const TailTable *tt = nullptr) const {
        EnvArgs E;
        E.ram_prev = ram_prev; E.ram_cur = ram_cur; E.stacks = stacks; E.T = tables;
        E.ret = ret; E.sign = sign; E.step_reward = step_reward; E.len = len; E.done = done; E.stepped = stepped; E.action = action; E.step_counter = nullptr;
        E.bc = bc; E.bc_mode = bc ? bc_mode : 0; E.bc_max_steps = cfg.bc_max_steps; E.immortal = k.dbg_immortal;
        E.spec_prev = spec_prev; E.spec_cur = spec_cur; E.spec_rw = spec_rw; E.spec_stacks = spec_stacks; E.spec_y1 = spec_y1;
        set_tail_table(E, tt);
        return E;
    }
    // what plan.h reads beyond the knobs
    PlanFacts facts() const {
        PlanFacts f{};
        f.dense_scale = dense_scale; f.kind = L.kind; f.members_materialized = members_materialized; f.uniform_base = uniform_base;
        f.antithetic_slot0 = antithetic_slot0; f.pair_sigma_uniform = pair_sigma_uniform; f.n_streams = (int)sub_streams.size();
        f.has_y3s = y3s != nullptr; f.has_theta_perm = theta_perm != nullptr; f.has_scaled_table = noise_pre != nullptr;
        return f;
    }
    hipEvent_t event(size_t i) {
        while (ev_pool.size() <= i) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            ev_pool.push_back(e);
        }
        return ev_pool[i];
    }
};

static int rec_reserve(dne_handle *h, int n_global, int per_world);

// the two small scratch arrays (scratch_f floats, scratch_i int64s) hold at least n elements each afterwards; contents are not kept
static int scratch_reserve(dne_handle *h, size_t n) {
    if (n <= h->scratch_cap) return 0;
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = h->release(h->scratch_f);
    if (e == hipSuccess) e = h->release(h->scratch_i);
    h->scratch_cap = 0;
    const size_t cap = std::max<size_t>(n, 65536);
    if (e == hipSuccess) e = h->alloc(&h->scratch_f, cap, "scratch_f");
    if (e == hipSuccess) e = h->alloc(&h->scratch_i, cap, "scratch_i");
    if (e != hipSuccess) return h->fail("scratch_reserve(%zu): %s", n, hipGetErrorString(e));
    h->scratch_cap = cap;
    return 0;
}

// Every entry point runs on the handle's device whatever the calling thread's current device is, and puts the
// caller's device back on the way out.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(const dne_handle *h) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != h->cfg.device_id) hipSetDevice(h->cfg.device_id); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};

// the four whole-episode kinds by name, and the one spelling of "this call is another kind's"
static_assert(DNE_KIND_CARTPOLE == DNE_KIND_MAZE + 1 && DNE_KIND_PENDULUM == DNE_KIND_MAZE + 2 && DNE_KIND_MJMAZE == DNE_KIND_MAZE + 3, "the table below");
static const char *episodic_kind_name(int kind) {
    static const char *const names[] = {"DNE_KIND_MAZE", "DNE_KIND_CARTPOLE", "DNE_KIND_PENDULUM", "DNE_KIND_MJMAZE"};
    if (kind == DNE_ENV_ACROBOT) return "DNE_ENV_ACROBOT";   // (an environment id: what a DNE_KIND_DENSE engine or a host twin steps)
    return names[kind - DNE_KIND_MAZE];
}
static int needs_kind(dne_handle *h, const char *call, int kind) {
    return h->L.kind == kind ? 0 : h->fail("%s needs a %s engine (this one: kind %d)", call, episodic_kind_name(kind), h->L.kind);
}

// f(the Options of the MujocoPolicy kind this handle is): the two types differ in the width of mean / std alone
template <class F> static void with_mujoco_options(dne_handle *h, F &&f) { if (h->mjmaze) f(h->mj_opt); else f(h->pd_opt); }

// an Options (pendulum: 3 observations, mjmaze: 11) from its parts; mean / std null: NaN, the policy before set_ob_stat (policies.py:138-141)
template <class Options>
static void fill_options(Options &o, int n_out, int ac_mode, float ac_noise_std, const float *mean, const float *std) {
    o.n_out = n_out; o.ac_mode = ac_mode; o.ac_noise_std = ac_noise_std;
    for (size_t i = 0; i < sizeof(o.mean) / sizeof(float); i++) { o.mean[i] = mean ? mean[i] : NAN; o.std[i] = std ? std[i] : NAN; }
}

static void make_layout(int kind, int nact, Layout *L) {
    int o = 0;
    memset(L, 0, sizeof(*L));
    L->kind = kind; L->nact = nact;
    auto take = [&](int n) { int r = o; o += n; return r; };
    if (kind == DNE_KIND_MAZE || kind == DNE_KIND_CARTPOLE || kind == DNE_KIND_PENDULUM || kind == DNE_KIND_MJMAZE || kind == DNE_KIND_DENSE) {   // (DNE_KIND_PENDULUM, DNE_KIND_MJMAZE, DNE_KIND_DENSE: P depends on the hidden width, dne_create sets it) SimpleClassifier (models/simple.py:29-35): csrc/maze.h and csrc/cartpole.h hold its offsets
        L->c1w = L->c1b = L->c2w = L->c2b = L->c3w = L->c3b = L->fcw = L->fcb = L->ow = L->ob = -1;
        L->bn1b = L->bn1g = L->bn2b = L->bn2g = L->bn3b = L->bn3g = -1;
        o = kind == DNE_KIND_MAZE ? maze::NPARAMS : kind == DNE_KIND_CARTPOLE ? cartpole::NPARAMS : 0;
    } else if (kind == DNE_KIND_ES) {   // creation order of trainable variables, policies.py:319-330
        L->c1w = take(4096); L->c1b = take(16); L->bn1b = take(16); L->bn1g = take(16);
        L->c2w = take(8192); L->c2b = take(32); L->bn2b = take(32); L->bn2g = take(32);
        L->fcw = take(3872 * 256); L->fcb = take(256); L->bn3b = take(256); L->bn3g = take(256);
        L->ow = take(256 * nact); L->ob = take(nact);
    } else if (kind == DNE_KIND_ES_VBN) {   // models/batchnorm.py:52-123, creation order (base.py:35-44): w, then BatchNorm/b
        L->c1w = take(4096); L->bn1b = take(16);
        L->c2w = take(8192); L->bn2b = take(32);
        L->fcw = take(3872 * 256); L->bn3b = take(256);
        L->ow = take(256 * nact); L->ob = take(nact);
        L->c1b = L->c2b = L->fcb = L->bn1g = L->bn2g = L->bn3g = -1;   // absent: +0.0f biases, 1.0f gammas (opt_bias / opt_gamma)
    } else if (kind == DNE_KIND_GA_LARGE) {   // models/dqn.py:39-47: variables in creation order (models/base.py:35-41)
        L->c1w = take(8 * 8 * 4 * 32); L->c1b = take(32); L->c2w = take(4 * 4 * 32 * 64); L->c2b = take(64);
        L->c3w = take(3 * 3 * 64 * 64); L->c3b = take(64);
        L->fcw = take(7744 * 512); L->fcb = take(512); L->ow = take(512 * nact); L->ob = take(nact);
        L->bn1b = L->bn1g = L->bn2b = L->bn2g = L->bn3b = L->bn3g = -1;
    } else {                     // policies.py:449-459 via tf_util.py:133-162
        L->c1w = take(4096); L->c1b = take(16); L->c2w = take(8192); L->c2b = take(32);
        L->fcw = take(3872 * 256); L->fcb = take(256); L->ow = take(256 * nact); L->ob = take(nact);
        L->bn1b = L->bn1g = L->bn2b = L->bn2g = L->bn3b = L->bn3g = -1;
    }
    L->P = o;
}

// Pillow Resample.c precompute_coeffs (BILINEAR, support 1.0) -- the filter WarpFrame uses
// (atari_wrappers.py:140-141); third-party algorithm restated from its published source.
static void pil_coeffs(int in_size, int out_size, int ksize, int *bounds, double *kk) {
    const double scale = (double)in_size / out_size;
    const double fscale = scale < 1.0 ? 1.0 : scale;
    const double support = fscale;
    for (int xx = 0; xx < out_size; xx++) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        if (xmax > ksize) { fprintf(stderr, "dne: a resize window of %d taps does not fit the table's %d\n", xmax, ksize); abort(); }
        double ww = 0.0;
        double *k = kk + xx * ksize;
        for (int x = 0; x < ksize; x++) k[x] = 0.0;
        for (int x = 0; x < xmax; x++) {
            double t = (x + xmin - center + 0.5) * (1.0 / fscale);
            t = t < 0 ? -t : t;
            k[x] = t < 1.0 ? 1.0 - t : 0.0;
            ww += k[x];
        }
        if (ww != 0.0)
            for (int x = 0; x < xmax; x++) k[x] /= ww;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

static const uint8_t kPalette[16][3] = {
    {0, 0, 0},       {170, 170, 170}, {45, 50, 184},   {24, 26, 167},  {214, 214, 214}, {0, 28, 136},
    {236, 236, 236}, {84, 138, 210},  {198, 108, 58},  {181, 83, 40},  {192, 192, 192}, {252, 252, 84},
    {92, 186, 92},   {74, 74, 74},    {252, 144, 144}, {0, 44, 160}};

static void make_tables(ResizeLds *T) {
    // Fixed RS_KH / RS_KV taps per output pixel (the widest window PIL builds for these two scales): windows that would leave the frame are
    // shifted back inside and their weights shifted with them, zero weights filling the rest (0 + x*0.0 and acc + x*0.0 are exact no-ops).
    double kh[84 * RS_KH], kv[84 * RS_KV];
    int bh[84 * 2], bv[84 * 2];
    pil_coeffs(160, 84, RS_KH, bh, kh);
    pil_coeffs(210, 84, RS_KV, bv, kv);
    memset(T, 0, sizeof(*T));
    for (int xx = 0; xx < 84; xx++) {
        const int x0 = bh[2 * xx], d = x0 + RS_KH > 160 ? x0 + RS_KH - 160 : 0;
        T->xmin[xx] = (uint8_t)(x0 - d);
        for (int t = 0; t < RS_KH; t++) T->kh[xx * RS_KH + t] = t >= d ? kh[xx * RS_KH + t - d] : 0.0;
    }
    for (int yy = 0; yy < 84; yy++) {
        const int y0 = bv[2 * yy], d = y0 + RS_KV > 210 ? y0 + RS_KV - 210 : 0;
        T->ymin[yy] = (uint8_t)(y0 - d);
        for (int t = 0; t < RS_KV; t++) T->kv[yy * RS_KV + t] = t >= d ? kv[yy * RS_KV + t - d] : 0.0;
    }
    for (int a = 0; a < 16; a++)
        for (int b = 0; b < 16; b++) {   // MaxAndSkip max (atari_wrappers.py:105) then WarpFrame gray (:139)
            const uint8_t r = std::max(kPalette[a][0], kPalette[b][0]);
            const uint8_t g = std::max(kPalette[a][1], kPalette[b][1]);
            const uint8_t bl = std::max(kPalette[a][2], kPalette[b][2]);
            volatile float t0 = (float)r * 0.299f, t1 = (float)g * 0.587f, t2 = (float)bl * 0.114f;
            volatile float s = t0 + t1;
            T->gray2[(a << 4) | b] = s + t2;
        }
}

template <typename T>
static hipError_t dalloc(T **p, size_t n) {
    return hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T));
}

// scratch device buffer of one call: freed on every exit path
template <typename T>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t alloc(size_t n) { return dalloc(&p, n); }
    operator T *() const { return p; }
};

// a refused shape of DNE_KIND_DENSE by name (code: dense::make_shape's answer); 0 for a shape that is built
static int dense_shape_error(const char *who, int code, int env, int n_hidden, const int32_t *widths, int n_widths, int nonlin, int n_out) {
    const std::string w(who);
    if (code == dense::SHAPE_OK) return 0;
    if (code == dense::SHAPE_ENV)
        g_create_error = w + " runs on the environments DNE_KIND_MAZE (4), DNE_KIND_CARTPOLE (5) and DNE_KIND_PENDULUM (6); environment " + std::to_string(env) + " is refused (DNE_ENV_ACROBOT (9) is the fourth)";
    else if (code == dense::SHAPE_LAYERS)
        g_create_error = w + " is built for 0.." + std::to_string(dense::MAX_HIDDEN) + " hidden layers; " + std::to_string(n_hidden) + " hidden layers are refused";
    else if (code == dense::SHAPE_WIDTH) {
        int i = 0;
        while (i < n_hidden - 1 && widths[i] >= 1 && widths[i] <= dense::MAX_WIDTH) i++;
        g_create_error = w + " is built for hidden widths 1.." + std::to_string(dense::MAX_WIDTH) + "; width " + std::to_string(widths[i]) + " of hidden layer " + std::to_string(i) + " is refused";
    } else if (code == dense::SHAPE_TAIL) {
        int i = n_hidden;
        while (i < n_widths - 1 && widths[i] == 0) i++;
        g_create_error = w + ": " + std::to_string(n_hidden) + " hidden layers, and a width of " + std::to_string(widths[i]) + " behind them (entry " + std::to_string(i) + "); unused widths are 0";
    } else if (code == dense::SHAPE_OUT)
        g_create_error = w + " has " + std::to_string(dense::env_outputs(env)) + " outputs on environment " + std::to_string(env) + " (the maze and the cart-pole 2, the pendulum 1, the acrobot 3), n_actions " + std::to_string(n_out) + " is refused";
    else
        g_create_error = w + " has nonlinearities 0 (tanh) and 1 (relu); nonlinearity " + std::to_string(nonlin) + " is refused";
    return -1;
}

extern "C" int dne_dense_num_params(int env_kind, int n_hidden, const int32_t *widths, int n_out) {
    dense::Shape sh;
    if (n_hidden > 0 && !widths) return -1;
    return dense::make_shape(env_kind, n_hidden, widths, n_hidden < 0 ? 0 : n_hidden, dense::NL_RELU, n_out, &sh) == dense::SHAPE_OK ? sh.P : -1;
}

extern "C" int dne_num_params(int kind, int nact) {
    if (kind == DNE_KIND_MAZE && nact != maze::ACT) return -1;   // the maze policy has two raw outputs, nothing else
    if (kind == DNE_KIND_CARTPOLE && nact != cartpole::ACT) return -1;   // CartPole-v1 has two actions
    if (kind == DNE_KIND_PENDULUM) return -1;   // P depends on the hidden width: dne_pendulum_num_params
    if (kind == DNE_KIND_MJMAZE) return -1;     // likewise: dne_mjmaze_num_params
    if (kind == DNE_KIND_DENSE) return -1;      // P depends on the whole shape: dne_dense_num_params
    if (kind == DNE_ENV_ACROBOT) return -1;     // an environment id, not a kind: dne_dense_num_params(DNE_ENV_ACROBOT, ...)
    Layout L;
    make_layout(kind, nact, &L);
    return L.P;
}

// the engine's knobs as dne_create reads them
static Knobs engine_knobs(int kind, int nact) { return knobs_from_env(kind, nact, SPEC_ACTIONS - 2); }

extern "C" int dne_debug_plan(int kind, int n_actions, const dne_plan_facts *facts, int total, int gsize, dne_window_plan *out, int cap,
                              int *nsub, int whole_eval) {
    if (kind == DNE_KIND_MAZE) {   // no lock-step to plan: one launch per evaluation
        g_create_error = "dne_debug_plan: a DNE_KIND_MAZE engine (kind 4) has no lock-step windows, an evaluation is one k_maze_rollout launch";
        return -1;
    }
    if (kind == DNE_KIND_CARTPOLE) {
        g_create_error = "dne_debug_plan: a DNE_KIND_CARTPOLE engine (kind 5) has no lock-step windows, an evaluation is one k_cartpole_rollout launch";
        return -1;
    }
    if (kind == DNE_KIND_PENDULUM) {
        g_create_error = "dne_debug_plan: a DNE_KIND_PENDULUM engine (kind 6) has no lock-step windows, an evaluation is one k_pendulum_rollout launch";
        return -1;
    }
    if (kind == DNE_KIND_MJMAZE) {
        g_create_error = "dne_debug_plan: a DNE_KIND_MJMAZE engine (kind 7) has no lock-step windows, an evaluation is one k_mjmaze_rollout launch";
        return -1;
    }
    if (kind == DNE_KIND_DENSE) {
        g_create_error = "dne_debug_plan: a DNE_KIND_DENSE engine (kind 8) has no lock-step windows, an evaluation is one k_dense_run launch";
        return -1;
    }
    const Knobs k = engine_knobs(kind, n_actions);
    PlanFacts f = *facts;
    f.kind = kind;
    const StepPlan p = plan_step(k, f, total, gsize, whole_eval != 0);
    if (nsub) *nsub = p.nsub;
    if (whole_eval) return fc_full_kind(p);
    for (int s = 0; s < p.nsub && s < cap; s++) {
        const Window c = window(total, p.nsub, s);
        out[s] = plan_window(k, f, p, total, c.cnt, gsize, true);
        out[s].lo = c.lo;
    }
    return 0;
}

extern "C" int dne_debug_plan_act(int kind, int n_actions, const dne_plan_facts *facts, int n, dne_window_plan *out) {
    if (kind == DNE_KIND_MAZE) {   // dne_act refuses the kind
        g_create_error = "dne_debug_plan_act: a DNE_KIND_MAZE engine (kind 4) has no dne_act";
        return -1;
    }
    if (kind == DNE_KIND_CARTPOLE) {
        g_create_error = "dne_debug_plan_act: a DNE_KIND_CARTPOLE engine (kind 5) has no dne_act";
        return -1;
    }
    if (kind == DNE_KIND_PENDULUM) {
        g_create_error = "dne_debug_plan_act: a DNE_KIND_PENDULUM engine (kind 6) has no dne_act";
        return -1;
    }
    if (kind == DNE_KIND_MJMAZE) {
        g_create_error = "dne_debug_plan_act: a DNE_KIND_MJMAZE engine (kind 7) has no dne_act";
        return -1;
    }
    if (kind == DNE_KIND_DENSE) {
        g_create_error = "dne_debug_plan_act: a DNE_KIND_DENSE engine (kind 8) has no dne_act (dne_stepenv_act is its forward pass)";
        return -1;
    }
    if (n < 1) {
        g_create_error = "dne_debug_plan_act: n must be at least 1";
        return -1;
    }
    PlanFacts f = *facts;
    f.kind = kind;
    *out = act_window(engine_knobs(kind, n_actions), f, n);
    return 0;
}

extern "C" int dne_debug_knob(int kind, int n_actions, const char *name) {
    const Knobs k = engine_knobs(kind, n_actions);
    for (const KnobRow &r : KNOBS)
        if (!strcmp(r.env, name)) return k.*r.field;
    return -1;
}

extern "C" const char *dne_last_error(dne_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

constexpr size_t ZERO_ROWS_FLOATS = 8 * 256;            // a row block of zeros (8 KB): k_fc_sub's dead rows (forward.h)
constexpr size_t OVERFETCH_FLOATS = 2 * 8 * 256 + 64;   // one row block of the streaming fc + the 64 floats of slack the table always had
static int grow_bases(dne_handle *h, int cap) {
    if (cap <= h->base_cap) return 0;
    float *nb = nullptr;
    HCHECK(h, h->alloc(&nb, (size_t)cap * h->base_stride + OVERFETCH_FLOATS, "bases"));   // (the same over-fetch behind the last slot)
    HCHECK(h, hipMemsetAsync(nb + (size_t)cap * h->base_stride, 0, OVERFETCH_FLOATS * sizeof(float), h->stream));
    if (h->bases) {
        HCHECK(h, hipMemcpyAsync(nb, h->bases, (size_t)h->base_cap * h->base_stride * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        HCHECK(h, hipStreamSynchronize(h->stream));
        HCHECK(h, h->release(h->bases));
    }
    for (int s = cap - 1; s >= std::max(h->base_cap, 1); s--) h->free_slots.push_back(s);
    h->bases = nb;
    h->base_cap = cap;
    return 0;
}

// A base slot above 0 the caller writes (dne_set_theta, dne_ga_rebuild, dne_ga_rebuild_powers) is the caller's from then on: the GA store
// neither hands it out again nor goes on believing that it holds what the store once put there.  A parent cached in it is forgotten
// (its chain is rebuilt elsewhere when next needed), and it is no longer a slot for materialised children.  dne_ga_set_init_scale
// takes every slot but 0 back.
static void claim_slot(dne_handle *h, int slot) {
    if (slot < 1) return;
    h->free_slots.erase(std::remove(h->free_slots.begin(), h->free_slots.end(), slot), h->free_slots.end());
    h->child_slots.erase(std::remove(h->child_slots.begin(), h->child_slots.end(), slot), h->child_slots.end());
    for (auto it = h->ga_cache.begin(); it != h->ga_cache.end();) {
        if (it->second == slot) it = h->ga_cache.erase(it);
        else ++it;
    }
}

extern "C" int dne_create(const dne_config *cfg, dne_handle **out) {
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_create_error = "dne_create: no HIP device visible (this engine has no CPU fallback)";
        return -1;
    }
    if (cfg->max_members <= 0 || (cfg->n_actions <= 1 && !(cfg->policy_kind == DNE_KIND_PENDULUM && cfg->n_actions == 1) && cfg->policy_kind != DNE_KIND_DENSE) ||
        (!es_like(cfg->policy_kind) && cfg->policy_kind != DNE_KIND_GA && cfg->policy_kind != DNE_KIND_GA_LARGE && cfg->policy_kind != DNE_KIND_MAZE &&
         cfg->policy_kind != DNE_KIND_CARTPOLE && cfg->policy_kind != DNE_KIND_PENDULUM && cfg->policy_kind != DNE_KIND_MJMAZE && cfg->policy_kind != DNE_KIND_DENSE)) {
        g_create_error = "dne_create: bad config";
        return -1;
    }
    // SynthAtari defines 18 actions (ALE order; a narrower engine uses the first n_actions of them), and the oracle's tables end there: a
    // wider head could pick an action nothing defines and no parity covers
    if (cfg->n_actions > 18) {
        g_create_error = "dne_create: n_actions " + std::to_string(cfg->n_actions) + " is outside 2..18: the SynthAtari fixture defines 18 actions";
        return -1;
    }
    if (cfg->policy_kind == DNE_KIND_MAZE && cfg->n_actions != maze::ACT) {
        g_create_error = "dne_create: DNE_KIND_MAZE has 2 outputs (the navigator's turn and speed), n_actions " + std::to_string(cfg->n_actions) + " is refused";
        return -1;
    }
    if (cfg->policy_kind == DNE_KIND_MAZE && cfg->bc_final_only) {
        g_create_error = "dne_create: bc_final_only is not available on a DNE_KIND_MAZE engine (kind 4): its bc rows are (x, y) after every step; "
                         "dne_maze_final_state has the final position of every member";
        return -1;
    }
    if (cfg->policy_kind == DNE_KIND_CARTPOLE && cfg->n_actions != cartpole::ACT) {
        g_create_error = "dne_create: DNE_KIND_CARTPOLE has 2 actions (push the cart left or right), n_actions " + std::to_string(cfg->n_actions) + " is refused";
        return -1;
    }
    if (cfg->policy_kind == DNE_KIND_CARTPOLE && cfg->bc_final_only) {
        g_create_error = "dne_create: bc_final_only is not available on a DNE_KIND_CARTPOLE engine (kind 5): it records no behaviour; "
                         "dne_cartpole_final_state has the final state of every member";
        return -1;
    }
    if (cfg->policy_kind == DNE_KIND_PENDULUM) {   // the shape: reserved[0] hidden width, [1] action mode, [2] nonlinearity; n_actions = the outputs
        const int hidden = cfg->reserved[0], mode = cfg->reserved[1], nl = cfg->reserved[2];
        if (!pendulum::hidden_ok(hidden)) {
            g_create_error = "dne_create: DNE_KIND_PENDULUM is built for two hidden layers of width 64, 128 or 256; hidden width " + std::to_string(hidden) + " is refused";
            return -1;
        }
        if (mode != pendulum::AC_CONTINUOUS && mode != pendulum::AC_UNIFORM) {
            g_create_error = "dne_create: DNE_KIND_PENDULUM has action modes 0 (continuous) and 1 (uniform bins); mode " + std::to_string(mode) + " is refused";
            return -1;
        }
        if (nl != pendulum::NL_TANH && nl != pendulum::NL_RELU) {
            g_create_error = "dne_create: DNE_KIND_PENDULUM has nonlinearities 0 (tanh) and 1 (relu); nonlinearity " + std::to_string(nl) + " is refused";
            return -1;
        }
        if (mode == pendulum::AC_CONTINUOUS ? cfg->n_actions != 1 : (cfg->n_actions < 2 || cfg->n_actions > pendulum::MAX_OUT)) {
            g_create_error = "dne_create: DNE_KIND_PENDULUM has 1 output under the continuous action and 2..16 under uniform bins, n_actions " +
                             std::to_string(cfg->n_actions) + " under mode " + std::to_string(mode) + " is refused";
            return -1;
        }
        if (cfg->bc_final_only || cfg->record_bc) {
            g_create_error = "dne_create: record_bc / bc_final_only are not available on a DNE_KIND_PENDULUM engine (kind 6): it records no behaviour; "
                             "dne_pendulum_final_state has the final state of every member";
            return -1;
        }
    }
    if (cfg->policy_kind == DNE_KIND_MJMAZE) {   // the shape as on DNE_KIND_PENDULUM; n_actions = the outputs: 2, or 2 B
        const int hidden = cfg->reserved[0], mode = cfg->reserved[1], nl = cfg->reserved[2];
        if (!pendulum::hidden_ok(hidden)) {
            g_create_error = "dne_create: DNE_KIND_MJMAZE is built for two hidden layers of width 64, 128 or 256; hidden width " + std::to_string(hidden) + " is refused";
            return -1;
        }
        if (mode != pendulum::AC_CONTINUOUS && mode != pendulum::AC_UNIFORM) {
            g_create_error = "dne_create: DNE_KIND_MJMAZE has action modes 0 (continuous) and 1 (uniform bins); mode " + std::to_string(mode) + " is refused";
            return -1;
        }
        if (nl != pendulum::NL_TANH && nl != pendulum::NL_RELU) {
            g_create_error = "dne_create: DNE_KIND_MJMAZE has nonlinearities 0 (tanh) and 1 (relu); nonlinearity " + std::to_string(nl) + " is refused";
            return -1;
        }
        if (!mjmaze::shape_ok(hidden, cfg->n_actions, mode, nl)) {
            g_create_error = "dne_create: DNE_KIND_MJMAZE has 2 outputs under the continuous action and 2 B for B = 2..8 uniform bins a dimension, n_actions " +
                             std::to_string(cfg->n_actions) + " under mode " + std::to_string(mode) + " is refused";
            return -1;
        }
        if (cfg->bc_final_only || cfg->record_bc) {
            g_create_error = "dne_create: record_bc / bc_final_only are not available on a DNE_KIND_MJMAZE engine (kind 7): its behaviour characterisation is "
                             "the final (x, y), and dne_maze_final_state has it for every member";
            return -1;
        }
    }
    dense::Shape dn_shape{};
    if (cfg->policy_kind == DNE_KIND_DENSE) {   // the shape: reserved[0] the environment, [1] hidden layers, [2] nonlinearity, [3..5] the widths; n_actions = the outputs
        if (dense_shape_error("dne_create: DNE_KIND_DENSE", dense::make_shape(cfg->reserved[0], cfg->reserved[1], cfg->reserved + 3, 3, cfg->reserved[2], cfg->n_actions, &dn_shape),
                              cfg->reserved[0], cfg->reserved[1], cfg->reserved + 3, 3, cfg->reserved[2], cfg->n_actions)) return -1;
        if (cfg->bc_final_only || cfg->record_bc) {
            g_create_error = "dne_create: record_bc / bc_final_only are not available on a DNE_KIND_DENSE engine (kind 8): it records no behaviour; "
                             "dne_dense_final_state has the final state of every member";
            return -1;
        }
    }
    dne_handle *h = new dne_handle();
    h->cfg = *cfg;
    auto bail = [&](int) { g_create_error = h->err; delete h; return -1; };
#define CCHECK(expr) do { if ((expr) != 0) return bail(0); } while (0)
#define CH(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { h->fail("%s -> %s", #expr, hipGetErrorString(_e)); return bail(0); } } while (0)
    CH(hipSetDevice(cfg->device_id));
    CH(hipStreamCreate(&h->stream));
    h->sub_streams.push_back(h->stream);
    // the diagnosis switches (the scheduling and tuning knobs: plan.h)
    auto env_int = [](const char *name, int lo, int hi, int *dst) {
        if (const char *e = getenv(name)) *dst = std::max(lo, std::min(hi, atoi(e)));
    };
    {
        int rz = 1, tr = 0, ds = 0;
        env_int("DNE_REDZONE", 0, 1, &rz); env_int("DNE_TRACE", 0, 1, &tr); env_int("DNE_DEBUG_SYNC", 0, 1, &ds);
        h->redzone = rz ? 4096 : 0; h->trace_on = tr != 0; h->debug_sync = ds != 0;
        int sc = 1;
        env_int("DNE_STAGED_COPY", 0, 1, &sc);
        h->staged_copies = sc != 0;
    }
    if (cfg->policy_kind == DNE_KIND_MAZE || cfg->policy_kind == DNE_KIND_CARTPOLE || cfg->policy_kind == DNE_KIND_PENDULUM || cfg->policy_kind == DNE_KIND_MJMAZE ||
        cfg->policy_kind == DNE_KIND_DENSE) {
        // theta slots, member descriptors and accumulators, the walls (the cart-pole: seeds and final states), the reduce and optimizer
        // buffers: no frame, activation or ring buffer
        h->maze = cfg->policy_kind == DNE_KIND_MAZE;
        h->cartpole = cfg->policy_kind == DNE_KIND_CARTPOLE;
        h->pendulum = cfg->policy_kind == DNE_KIND_PENDULUM;
        h->mjmaze = cfg->policy_kind == DNE_KIND_MJMAZE;
        h->dense = cfg->policy_kind == DNE_KIND_DENSE;
        const bool mujoco = h->pendulum || h->mjmaze;
        make_layout(cfg->policy_kind, cfg->n_actions, &h->L);
        if (mujoco) {
            h->pd_hidden = cfg->reserved[0]; h->pd_nl = cfg->reserved[2];
            with_mujoco_options(h, [&](auto &o) { fill_options(o, cfg->n_actions, cfg->reserved[1], 0.0f, nullptr, nullptr); });
            h->L.P = h->mjmaze ? mjmaze::offsets(h->pd_hidden, cfg->n_actions).P : pendulum::offsets(h->pd_hidden, cfg->n_actions).P;
        }
        if (h->dense) { h->dn_shape = dn_shape; h->L.P = dn_shape.P; }
        h->M = cfg->max_members;
        h->base_stride = ((size_t)h->L.P + 63) / 64 * 64;
        const size_t M = h->M;
        CCHECK(grow_bases(h, 1));
        CH(hipMemset(h->bases, 0, h->base_stride * sizeof(float)));
        CH(h->alloc(&h->opt_m, h->L.P, "opt_m")); CH(h->alloc(&h->opt_v, h->L.P, "opt_v")); CH(h->alloc(&h->g, h->L.P, "g"));
        CH(hipMemset(h->opt_m, 0, h->L.P * sizeof(float))); CH(hipMemset(h->opt_v, 0, h->L.P * sizeof(float)));
        CH(h->alloc(&h->partial, 2 * ((size_t)h->L.P / 256 + 1), "partial"));
        CH(h->alloc(&h->m_slot, M, "m_slot")); CH(h->alloc(&h->m_off, M, "m_off")); CH(h->alloc(&h->m_scale, M, "m_scale"));
        CH(hipMemset(h->m_slot, 0, M * sizeof(int32_t))); CH(hipMemset(h->m_off, 0, M * sizeof(int64_t))); CH(hipMemset(h->m_scale, 0, M * sizeof(float)));
        CH(h->alloc(&h->ret, M, "ret")); CH(h->alloc(&h->sign, M, "sign")); CH(h->alloc(&h->len, M, "len"));
        CH(hipMemset(h->ret, 0, M * sizeof(float))); CH(hipMemset(h->sign, 0, M * sizeof(float))); CH(hipMemset(h->len, 0, M * sizeof(int32_t)));
        if (h->dense) {   // the final state records, the seeds, and the walls when the environment is the maze
            stepenv::Dims d{};
            stepenv::dims(dn_shape.env, &d);
            CH(h->alloc(&h->dn_state, (size_t)d.state * M, "dense_state")); CH(h->alloc(&h->seeds, M, "seeds"));
            CH(hipMemset(h->dn_state, 0, (size_t)d.state * M * sizeof(double))); CH(hipMemset(h->seeds, 0, M * sizeof(uint32_t)));
            if (dn_shape.env == DNE_KIND_MAZE) CH(h->alloc(&h->maze_walls, maze::MAX_WALLS * 4, "maze_walls"));
        } else if (h->maze || h->mjmaze) {
            CH(h->alloc(&h->maze_xy, 2 * M, "maze_xy")); CH(h->alloc(&h->maze_walls, maze::MAX_WALLS * 4, "maze_walls"));
            CH(hipMemset(h->maze_xy, 0, 2 * M * sizeof(float)));
        } else {   // the kinds that reset from a seed: the final state's doubles (the cart-pole: 4, the pendulum: 2) and the seeds
            double *&state = h->cartpole ? h->cp_state : h->pd_state;
            const size_t S = h->cartpole ? 4 : 2;
            CH(h->alloc(&state, S * M, h->cartpole ? "cartpole_state" : "pendulum_state")); CH(h->alloc(&h->seeds, M, "seeds"));
            CH(hipMemset(state, 0, S * M * sizeof(double))); CH(hipMemset(h->seeds, 0, M * sizeof(uint32_t)));
        }
        if (mujoco) {   // the statistics and the per-member options, under the kind's own block names
            dne_handle::MujocoOptions &O = h->mo;
            const size_t W = h->mjmaze ? mjmaze::OBS : pendulum::OBS;
            const std::string kind = h->mjmaze ? "mjmaze" : "pendulum";
            CH(h->alloc(&O.sum, W * M, (kind + "_ob_sum").c_str())); CH(h->alloc(&O.sumsq, W * M, (kind + "_ob_sumsq").c_str())); CH(h->alloc(&O.count, M, (kind + "_ob_count").c_str()));
            CH(h->alloc(&O.off, M, (kind + "_ac_off").c_str())); CH(h->alloc(&O.flag, M, (kind + "_stat_flag").c_str()));
            CH(hipMemset(O.sum, 0, W * M * sizeof(double))); CH(hipMemset(O.sumsq, 0, W * M * sizeof(double))); CH(hipMemset(O.count, 0, M * sizeof(int32_t)));
            CH(hipMemset(O.off, 0xff, M * sizeof(int64_t))); CH(hipMemset(O.flag, 0, M));
        }
        if (h->maze && cfg->record_bc) {   // behaviour: the navigator's (x, y) after every step, [member][bc_max_steps][2] floats
            h->bc_bytes = M * (size_t)std::max(cfg->bc_max_steps, 1) * 2 * sizeof(float);
            CH(h->alloc(&h->bc, h->bc_bytes, "bc"));
            CH(hipMemset(h->bc, 0, h->bc_bytes));
        }
        h->scratch_cap = std::max<size_t>(4 * M + 64, 65536);
        CH(h->alloc(&h->scratch_f, h->scratch_cap, "scratch_f")); CH(h->alloc(&h->scratch_i, h->scratch_cap, "scratch_i"));
        CH(hipEventCreate(&h->ev_a)); CH(hipEventCreate(&h->ev_b));
        CH(hipDeviceSynchronize());
        h->trace("engine created: kind %d (%s), %d members, %zu device buffers", cfg->policy_kind, h->maze ? "hard maze" : h->cartpole ? "cart-pole" : h->pendulum ? "pendulum" : h->dense ? "dense policy on a step environment" : "MujocoPolicy on the hard maze", h->M, h->blocks.size());
        *out = h;
        return 0;
    }
    h->k = engine_knobs(cfg->policy_kind, cfg->n_actions);
    CH(hipFuncSetAttribute((const void *)k_conv12<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Conv12Lds)));
    CH(hipFuncSetAttribute((const void *)k_conv12<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Conv12Lds)));
    CH(hipFuncSetAttribute((const void *)k_conv12t<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Conv12Lds)));
    CH(hipFuncSetAttribute((const void *)k_conv12t<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Conv12Lds)));
    CH(hipFuncSetAttribute((const void *)k_unit_order, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CH(hipFuncSetAttribute((const void *)k_fc_ref<4>, hipFuncAttributeMaxDynamicSharedMemorySize, FCREF4_LDS));   // the running fold
    CH(hipFuncSetAttribute((const void *)k_lconv_mfma<32, 64, 4, 2, 21, 11, 1, 34, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lconv_mfma_lds_bytes<32, 4, 2, 11, 34>()));
    CH(hipFuncSetAttribute((const void *)k_lconv_mfma<64, 64, 3, 1, 11, 11, 1, 68, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lconv_mfma_lds_bytes<64, 3, 1, 11, 68>()));
    CH(hipFuncSetAttribute((const void *)k_lconv_mfma<32, 64, 4, 2, 21, 11, 1, 34, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lconv_mfma_lds_bytes<32, 4, 2, 11, 34>()));
    CH(hipFuncSetAttribute((const void *)k_lconv_mfma<64, 64, 3, 1, 11, 11, 1, 68, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lconv_mfma_lds_bytes<64, 3, 1, 11, 68>()));
    {   // k_out: the staged output weights (66 KB for a pair at 32 actions) or the DNE_OUT_LDS_KB reservation, whichever is larger
        constexpr int out_lds_max = (int)std::max(out_stage_bytes(2, OUT_NA), (size_t)64 * 1024);
        const void *outs[] = {(const void *)k_out<1, false, OUT_NA_ATARI>, (const void *)k_out<1, true, OUT_NA_ATARI>, (const void *)k_out<2, false, OUT_NA_ATARI>,
                              (const void *)k_out<2, true, OUT_NA_ATARI>,  (const void *)k_out<1, false, OUT_NA>,      (const void *)k_out<1, true, OUT_NA>,
                              (const void *)k_out<2, false, OUT_NA>,       (const void *)k_out<2, true, OUT_NA>};
        for (const void *f : outs) CH(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, out_lds_max));
    }
#ifdef DNE_PHASE_CLOCK
    {
        int burn = 0;
        env_int("DNE_ENV_BURN", 0, 1 << 20, &burn);
        CH(hipMemcpyToSymbol(HIP_SYMBOL(g_env_burn), &burn, sizeof(int)));
    }
#endif
    for (int s = 1; s < N_STREAMS; s++) { hipStream_t st; CH(hipStreamCreate(&st)); h->sub_streams.push_back(st); }
    make_layout(cfg->policy_kind, cfg->n_actions, &h->L);
    h->M = cfg->max_members;
    h->F = es_like(cfg->policy_kind) ? (cfg->ref_count > 0 ? cfg->ref_count : 128) : 0;
    if (h->F % 8) { h->fail("ref_count must be a multiple of 8"); return bail(0); }
    h->ref_chunk = cfg->ref_chunk > 0 ? cfg->ref_chunk : 512;
    h->ref_chunk = std::min(h->ref_chunk, h->M);
    h->base_stride = ((size_t)h->L.P + 63) / 64 * 64;
    const size_t M = h->M;
    CCHECK(grow_bases(h, 1));
    CH(hipMemset(h->bases, 0, h->base_stride * sizeof(float)));
    CH(h->alloc(&h->opt_m, h->L.P, "opt_m")); CH(h->alloc(&h->opt_v, h->L.P, "opt_v")); CH(h->alloc(&h->g, h->L.P, "g"));
    CH(hipMemset(h->opt_m, 0, h->L.P * sizeof(float))); CH(hipMemset(h->opt_v, 0, h->L.P * sizeof(float)));
    CH(h->alloc(&h->partial, 2 * ((size_t)h->L.P / 256 + 1), "partial"));
    if (h->F) CH(h->alloc(&h->ref, (size_t)h->F * OB_BYTES, "ref"));
    if (h->F) CH(h->alloc(&h->ref_f32, (size_t)h->F * RF_FRAME, "ref_f32"));
    CH(hipFuncSetAttribute((const void *)k_conv1_ref_shared<16>, hipFuncAttributeMaxDynamicSharedMemorySize, RF_FRAME * (int)sizeof(float)));
    CH(hipFuncSetAttribute((const void *)k_conv1_ref_shared<8>, hipFuncAttributeMaxDynamicSharedMemorySize, RF_FRAME * (int)sizeof(float)));
    CH(hipFuncSetAttribute((const void *)k_conv2_ref_uniq, hipFuncAttributeMaxDynamicSharedMemorySize, C2U_LDS));
    if (h->k.ref_dedup && ref_default_route(h->k, h->F)) {   // room for every batch the dedup route takes (ref_dedup_pays)
        h->ref_cap1 = ref_pad(h->F * RI_N1, REF_U1_PAD);
        h->ref_cap2 = ref_pad(h->F * RI_N2, REF_U2_PAD);
        CH(h->alloc(&h->ref_tab1, (size_t)h->ref_cap1 * 256, "ref_tab1")); CH(h->alloc(&h->ref_idx1, (size_t)h->F * 448, "ref_idx1"));
        CH(h->alloc(&h->ref_win, (size_t)h->ref_cap2 * 16, "ref_win")); CH(h->alloc(&h->ref_idx2, (size_t)h->F * 128, "ref_idx2"));
    }
    CH(h->alloc(&h->m_slot, M, "m_slot")); CH(h->alloc(&h->m_off, M, "m_off")); CH(h->alloc(&h->m_scale, M, "m_scale"));
    CH(hipMemset(h->m_slot, 0, M * sizeof(int32_t))); CH(hipMemset(h->m_off, 0, M * sizeof(int64_t)));
    CH(hipMemset(h->m_scale, 0, M * sizeof(float)));
    CH(h->alloc(&h->bn, M * 608, "bn")); CH(h->alloc(&h->bn_mom, M * 608, "bn_mom"));
    CH(h->alloc(&h->ram_prev, M * 128, "ram_prev")); CH(h->alloc(&h->ram_cur, M * 128, "ram_cur")); CH(h->alloc(&h->stacks, M * OB_BYTES, "stacks"));
    CH(hipMemset(h->stacks, 0, M * OB_BYTES));
    CH(h->alloc(&h->tables, 1, "tables"));
    {
        ResizeLds T;
        make_tables(&T);
        CH(hipMemcpy(h->tables, &T, sizeof(T), hipMemcpyHostToDevice));
    }
    CH(h->alloc(&h->ret, M, "ret")); CH(h->alloc(&h->sign, M, "sign")); CH(h->alloc(&h->step_reward, M, "step_reward"));
    CH(h->alloc(&h->logits, M * cfg->n_actions, "logits"));
    CH(h->alloc(&h->len, M, "len")); CH(h->alloc(&h->done, M, "done")); CH(h->alloc(&h->action, M, "action")); CH(h->alloc(&h->seeds, M, "seeds")); CH(h->alloc(&h->stepped, M, "stepped"));
    CH(hipMemset(h->done, 0, M * sizeof(int32_t))); CH(hipMemset(h->len, 0, M * sizeof(int32_t)));
    h->large = cfg->policy_kind == DNE_KIND_GA_LARGE;
    if (h->large) { CH(h->alloc(&h->y1, M * 14112, "y1")); CH(h->alloc(&h->y2, M * 7744, "y2")); CH(h->alloc(&h->y3, M * 7744, "y3")); CH(h->alloc(&h->y3t, M * 512, "y3t")); }
    else { CH(h->alloc(&h->y1, M * 7056, "y1")); CH(h->alloc(&h->y2, M * 3872 + 64, "y2"));   /* (+ 64: k_fc_ring fetches the eight activations behind a slice's end and never uses them) */ CH(h->alloc(&h->y3, M * 256, "y3")); CH(h->alloc(&h->y3t, M * 4 * 256, "y3t")); }
    CH(h->alloc(&h->unit_order, M * 4, "unit_order"));
    if (!h->large) {   // a dead row's load: uniform base + lane * 16 + an immediate of up to 3 KB, whichever of the two 4 KB halves of a block it stands for
        CH(h->alloc(&h->zero_rows, ZERO_ROWS_FLOATS, "zero_rows"));
        CH(hipMemset(h->zero_rows, 0, ZERO_ROWS_FLOATS * sizeof(float)));
    }
    if (!h->large && h->k.fc_sub) CH(h->alloc(&h->y3s, M * 32 * 256, "y3s"));
    if (!h->large && h->k.ring_on && es_like(cfg->policy_kind)) CH(h->alloc(&h->theta_perm, (size_t)(3872 + 16) * 256, "theta_perm"));
    if (h->k.spec_max > 0) {   // candidate outcomes of the speculative tail: [list position][action]
        const size_t rows = (size_t)h->k.spec_max * SPEC_ACTIONS;
        CH(h->alloc(&h->spec_prev, rows * 128, "spec_prev")); CH(h->alloc(&h->spec_cur, rows * 128, "spec_cur"));
        CH(h->alloc(&h->spec_rw, rows * 2, "spec_rw")); CH(h->alloc(&h->spec_stacks, rows * OB_BYTES, "spec_stacks"));
        CH(h->alloc(&h->spec_y1, rows * 7056, "spec_y1"));
        CH(hipMemset(h->spec_prev, 0, rows * 128)); CH(hipMemset(h->spec_cur, 0, rows * 128));   // RAM bytes past the live 40 stay zero
    }
    if (h->F) {
        const size_t rr = (size_t)h->ref_chunk * h->F;
        for (int w = 0; w < 2; w++) {
            CH(h->alloc(&h->y1r[w], rr * 7056, "y1r[w]")); CH(h->alloc(&h->y2r[w], rr * Y2_PAD_ROW, "y2r[w]")); CH(h->alloc(&h->y3pr[w], rr * 4 * 256, "y3pr[w]"));
            CH(h->alloc(&h->fr1[w], rr * 2 * 16, "fr1[w]")); CH(h->alloc(&h->fr2[w], rr * 2 * 32, "fr2[w]"));
            CH(hipEventCreateWithFlags(&h->ev_ref[w], hipEventDisableTiming));
        }
    }
    CH(h->alloc(&h->list_a, M, "list_a")); CH(h->alloc(&h->list_b, M, "list_b")); CH(h->alloc(&h->count_dev, 8 + TT_MAX, "count_dev"));
    CH(hipHostMalloc((void **)&h->count_host, (8 + TT_MAX) * sizeof(int), hipHostMallocDefault));
    if (cfg->record_bc) {
        h->bc_bytes = es_like(cfg->policy_kind) && !cfg->bc_final_only ? M * (size_t)std::max(cfg->bc_max_steps, 1) * 128 : M * 128;
        CH(h->alloc(&h->bc, h->bc_bytes, "bc"));
        CH(hipMemset(h->bc, 0, h->bc_bytes));   // the emulator writes the RAM_LIVE bytes of a row; the other bytes of the 128 stay zero for good
    }
    h->scratch_cap = std::max<size_t>(4 * M + 64, 65536);
    CH(h->alloc(&h->scratch_f, h->scratch_cap, "scratch_f")); CH(h->alloc(&h->scratch_i, h->scratch_cap, "scratch_i"));
    CH(hipEventCreate(&h->ev_a)); CH(hipEventCreate(&h->ev_b));
    for (int i = 0; i < 64; i++) { hipEvent_t ev; CH(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); h->fc_ring.push_back(ev); }
    CH(hipDeviceSynchronize());
#undef CH
#undef CCHECK
    {
        size_t tot = 0;
        for (auto &b : h->blocks) tot += b.bytes;
        h->trace("engine created: kind %d, %d members, %d reference frames, %zu device buffers, %.2f GB", cfg->policy_kind, h->M,
                 h->F, h->blocks.size(), tot / 1e9);
    }
    *out = h;
    return 0;
}

// Every device buffer sits between two 4 KiB zones filled with 0xA5 at allocation; a kernel that writes outside its
// buffer shows up here (reads cannot be seen).  Returns the number of damaged zones (0 = clean), -1 on a HIP error;
// dne_last_error names the first damaged buffer.
extern "C" int dne_check_redzones(dne_handle *h) {
    DeviceGuard dg(h);
    if (!h->redzone) return 0;
    HCHECK(h, hipDeviceSynchronize());
    const size_t rz = h->redzone;
    std::vector<uint8_t> host(2 * rz);
    int bad = 0;
    for (auto &b : h->blocks) {
        HCHECK(h, hipMemcpy(host.data(), b.raw, rz, hipMemcpyDeviceToHost));
        HCHECK(h, hipMemcpy(host.data() + rz, b.raw + rz + b.bytes, rz, hipMemcpyDeviceToHost));
        for (int side = 0; side < 2; side++) {
            size_t first = rz;
            for (size_t i = 0; i < rz; i++)
                if (host[side * rz + i] != 0xA5) { first = i; break; }
            if (first < rz) {
                if (!bad) h->fail("red zone %s buffer '%s' (%zu bytes) damaged at byte %zu", side ? "after" : "before", b.name.c_str(),
                                  b.bytes, side ? first : rz - first);
                bad++;
            }
        }
    }
    return bad;
}

static void comm_destroy(dne_handle *h);

extern "C" void dne_destroy(dne_handle *h) {
    if (!h) return;
    DeviceGuard dg(h);
    hipDeviceSynchronize();
    if (dne_check_redzones(h) > 0) fprintf(stderr, "libdne_hip: %s\n", h->err.c_str());
    comm_destroy(h);
    for (auto &b : h->blocks) hipFree(b.raw);
    h->blocks.clear();
    for (int i = 0; i < 2; i++) {
        if (h->stage_buf[i]) hipHostFree(h->stage_buf[i]);
        if (h->stage_ev[i]) hipEventDestroy(h->stage_ev[i]);
    }
    for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
    if (h->count_host) hipHostFree(h->count_host);
    for (hipEvent_t e : h->fc_ring) hipEventDestroy(e);
    for (hipEvent_t e : h->ev_ref) if (e) hipEventDestroy(e);
    if (h->se_ev_a) hipEventDestroy(h->se_ev_a);
    if (h->se_ev_b) hipEventDestroy(h->se_ev_b);
    if (h->ev_a) hipEventDestroy(h->ev_a);
    if (h->ev_b) hipEventDestroy(h->ev_b);
    for (size_t s = 1; s < h->sub_streams.size(); s++) hipStreamDestroy(h->sub_streams[s]);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

extern "C" int dne_get_profile(dne_handle *h, dne_profile *out) {
    *out = h->prof;
    return 0;
}

// ------------------------------------------------------------------------------- noise / theta
// Large transfers go through two engine-owned pinned buffers instead of handing the caller's pageable memory to the
// runtime (which, above 128 MiB, registers the caller's pages with the GPU and copies from them in place -- the only
// transfer of that kind in a generation's life is the 1 GB table upload).  Small copies keep using hipMemcpy.
constexpr size_t STAGE_BYTES = 32u << 20, STAGE_MIN = 64u << 20;

static int stage_init(dne_handle *h) {
    for (int i = 0; i < 2; i++) {
        if (!h->stage_buf[i]) HCHECK(h, hipHostMalloc((void **)&h->stage_buf[i], STAGE_BYTES, hipHostMallocDefault));
        if (!h->stage_ev[i]) HCHECK(h, hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming));
    }
    return 0;
}

static int copy_h2d(dne_handle *h, void *dst, const void *src, size_t bytes) {
    if (bytes < STAGE_MIN || !h->staged_copies) { HCHECK(h, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return 0; }
    if (stage_init(h)) return -1;
    size_t done = 0;
    for (int c = 0; done < bytes; c++) {
        const int b = c & 1;
        const size_t n = std::min(STAGE_BYTES, bytes - done);
        if (c >= 2) HCHECK(h, hipEventSynchronize(h->stage_ev[b]));   // the copy that last read this buffer
        memcpy(h->stage_buf[b], (const uint8_t *)src + done, n);
        HCHECK(h, hipMemcpyAsync((uint8_t *)dst + done, h->stage_buf[b], n, hipMemcpyHostToDevice, h->stream));
        HCHECK(h, hipEventRecord(h->stage_ev[b], h->stream));
        done += n;
    }
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

static int copy_d2h(dne_handle *h, void *dst, const void *src, size_t bytes) {
    if (bytes < STAGE_MIN || !h->staged_copies) { HCHECK(h, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return 0; }
    if (stage_init(h)) return -1;
    HCHECK(h, hipStreamSynchronize(h->stream));
    size_t issued = 0, drained = 0;
    for (int c = 0; drained < bytes; c++) {   // chunk c is copied out of its buffer while chunk c + 1 arrives in the other
        const int b = c & 1;
        if (c == 0) {
            const size_t n = std::min(STAGE_BYTES, bytes);
            HCHECK(h, hipMemcpyAsync(h->stage_buf[0], src, n, hipMemcpyDeviceToHost, h->stream));
            HCHECK(h, hipEventRecord(h->stage_ev[0], h->stream));
            issued = n;
        }
        const size_t mine = std::min(STAGE_BYTES, bytes - drained);
        if (issued < bytes) {
            const size_t n = std::min(STAGE_BYTES, bytes - issued);
            HCHECK(h, hipMemcpyAsync(h->stage_buf[b ^ 1], (const uint8_t *)src + issued, n, hipMemcpyDeviceToHost, h->stream));
            HCHECK(h, hipEventRecord(h->stage_ev[b ^ 1], h->stream));
            issued += n;
        }
        HCHECK(h, hipEventSynchronize(h->stage_ev[b]));
        memcpy((uint8_t *)dst + drained, h->stage_buf[b], mine);
        drained += mine;
    }
    return 0;
}

extern "C" int dne_noise_alloc(dne_handle *h, size_t count) {
    DeviceGuard dg(h);
    if (count == 0) return h->fail("dne_noise_alloc: empty table");
    HCHECK(h, h->release(h->noise));
    HCHECK(h, h->release(h->noise_pre));
    h->noise_count = 0; h->noise_pre_count = 0;
    // the streaming fc kernels (k_fc_duo, k_fc_sub) fetch one 8-row block past a unit's last row and never use it: for small action
    // counts that block ends behind the member's parameter slice, i.e. up to OVERFETCH_FLOATS behind the table's last legal slice
    HCHECK(h, h->alloc(&h->noise, count + OVERFETCH_FLOATS, "noise"));
    HCHECK(h, hipMemset(h->noise + count, 0, OVERFETCH_FLOATS * sizeof(float)));
    h->noise_count = count;
    h->trace("noise table allocated: %zu floats", count);
    return 0;
}

extern "C" int dne_noise_write(dne_handle *h, size_t offset, const float *host, size_t count) {
    DeviceGuard dg(h);
    if (!h->noise || offset + count > h->noise_count) return h->fail("dne_noise_write: [%zu, %zu) outside the table of %zu", offset, offset + count, h->noise_count);
    h->noise_pre_count = 0;   // the scaled copy is stale
    return copy_h2d(h, h->noise + offset, host, count * sizeof(float));
}

extern "C" int dne_noise_upload(dne_handle *h, const float *host, size_t count) {
    if (dne_noise_alloc(h, count)) return -1;
    if (dne_noise_write(h, 0, host, count)) return -1;
    h->trace("noise table uploaded");
    return 0;
}

static int check_noise_range(dne_handle *h, int64_t idx, int64_t dim) {
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    if (idx < 0 || (uint64_t)(idx + dim) > h->noise_count) return h->fail("noise index %lld + %lld outside the table of %zu", (long long)idx, (long long)dim, h->noise_count);
    return 0;
}

extern "C" int dne_noise_get(dne_handle *h, int64_t idx, int dim, float *out) {
    DeviceGuard dg(h);
    if (check_noise_range(h, idx, dim)) return -1;
    HCHECK(h, hipMemcpy(out, h->noise + idx, (size_t)dim * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dne_set_theta(dne_handle *h, int slot, const float *theta, size_t n) {
    DeviceGuard dg(h);
    if (n != (size_t)h->L.P) return h->fail("dne_set_theta: expected %d parameters, got %zu", h->L.P, n);
    if (slot < 0) return h->fail("bad slot");
    if (grow_bases(h, slot + 1)) return -1;
    claim_slot(h, slot);
    HCHECK(h, hipMemcpy(h->bases + (size_t)slot * h->base_stride, theta, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int dne_get_theta(dne_handle *h, int slot, float *out, size_t n) {
    DeviceGuard dg(h);
    if (n != (size_t)h->L.P) return h->fail("dne_get_theta: expected %d parameters, got %zu", h->L.P, n);
    if (slot < 0 || slot >= h->base_cap) return h->fail("bad slot");
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, h->bases + (size_t)slot * h->base_stride, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dne_set_ref_batch(dne_handle *h, const uint8_t *ref, int count) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_set_ref_batch");
    if (!es_like(h->L.kind)) return h->fail("reference batch is an ESAtariPolicy concept");
    if (count != h->F) return h->fail("dne_set_ref_batch: engine was created for %d reference frames, got %d", h->F, count);
    HCHECK(h, hipMemcpy(h->ref, ref, (size_t)count * OB_BYTES, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_ref_to_float, dim3((count * RF_FRAME + 255) / 256), dim3(256), 0, h->stream, (const uint8_t *)h->ref, count, h->ref_f32);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->ref_dedup = false;
    if (h->ref_cap1) {
        RefIndex R;
        build_ref_index(ref, count, &R);
        const int U1p = ref_pad(R.U1, REF_U1_PAD), U2p = ref_pad(R.U2, REF_U2_PAD);
        // (ref_dedup_pays: few enough distinct rows, and y1u and y2u of a chunk fit beside each other in its y1r)
        const bool dedup = ref_dedup_pays(count, R.U1, R.U2) && U1p <= h->ref_cap1 && U2p <= h->ref_cap2;
        h->trace("reference batch: conv1 U1/N1 = %d/%d (%.1f %%), conv2 U2/N2 = %d/%d (%.1f %%): %s route", R.U1, count * RI_N1,
                 100.0 * R.U1 / (count * RI_N1), R.U2, count * RI_N2, 100.0 * R.U2 / (count * RI_N2), dedup ? "dedup" : "dense");
        h->ref_U1 = R.U1; h->ref_U2 = R.U2; h->ref_U1p = U1p; h->ref_U2p = U2p;
        if (dedup) {
            float lut[256];
            for (int i = 0; i < 256; i++) lut[i] = (float)i / 255.0f;   // k_ref_to_float's conversion
            std::vector<float> tab((size_t)U1p * 256, 0.0f);
            for (size_t i = 0; i < (size_t)R.U1 * 256; i++) tab[i] = lut[R.patches[i]];
            std::vector<int32_t> i1((size_t)count * 448, 0), win((size_t)U2p * 16, -1), i2((size_t)count * 128, 0);
            for (int f = 0; f < count; f++) {
                memcpy(&i1[(size_t)f * 448], &R.idx1[(size_t)f * RI_N1], RI_N1 * sizeof(int32_t));
                for (int p = 0; p < 128; p++) i2[(size_t)f * 128 + p] = R.idx2[(size_t)f * RI_N2 + std::min(p, RI_N2 - 1)];
            }
            memcpy(win.data(), R.windows.data(), R.windows.size() * sizeof(int32_t));
            HCHECK(h, hipMemcpy(h->ref_tab1, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
            HCHECK(h, hipMemcpy(h->ref_idx1, i1.data(), i1.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HCHECK(h, hipMemcpy(h->ref_win, win.data(), win.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HCHECK(h, hipMemcpy(h->ref_idx2, i2.data(), i2.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            h->ref_dedup = true;
        }
    }
    h->ref_set = true;
    return 0;
}

extern "C" int dne_ref_dedup_active(dne_handle *h, int *U1, int *U2) {
    if (!h->ref_set) return h->fail("reference batch not set (dne_set_ref_batch)");
    if (U1) *U1 = h->ref_cap1 ? h->ref_U1 : 0;
    if (U2) *U2 = h->ref_cap1 ? h->ref_U2 : 0;
    return h->ref_dedup ? 1 : 0;
}

// the index dne_set_ref_batch builds, on the CPU: no handle, no GPU (like dne_debug_plan)
extern "C" int dne_debug_ref_index(const uint8_t *ref, int count, int32_t *idx1, uint8_t *patches, int cap1, int32_t *idx2, int32_t *windows,
                                   int cap2, int *U1, int *U2) {
    if (!ref || count < 1) { g_create_error = "dne_debug_ref_index: no frames"; return -1; }
    RefIndex R;
    build_ref_index(ref, count, &R);
    if (U1) *U1 = R.U1;
    if (U2) *U2 = R.U2;
    if ((patches && cap1 < R.U1) || (windows && cap2 < R.U2)) { g_create_error = "dne_debug_ref_index: a table does not fit its capacity"; return -1; }
    if (idx1) memcpy(idx1, R.idx1.data(), R.idx1.size() * sizeof(int32_t));
    if (patches) memcpy(patches, R.patches.data(), R.patches.size());
    if (idx2) memcpy(idx2, R.idx2.data(), R.idx2.size() * sizeof(int32_t));
    if (windows) memcpy(windows, R.windows.data(), R.windows.size() * sizeof(int32_t));
    return ref_dedup_pays(count, R.U1, R.U2) ? 1 : 0;
}

extern "C" int dne_materialize(dne_handle *h, const int64_t *idx, int n, float sigma, float *out_host) {
    DeviceGuard dg(h);
    for (int i = 0; i < n; i++)
        if (check_noise_range(h, idx[i], h->L.P)) return -1;
    const size_t need = (size_t)n * 2 * h->L.P;
    if (need > h->mat_cap) {
        HCHECK(h, h->release(h->mat_out));
        HCHECK(h, h->alloc(&h->mat_out, need, "mat_out"));
        h->mat_cap = need;
    }
    if (scratch_reserve(h, (size_t)n)) return -1;
    HCHECK(h, hipMemcpyAsync(h->scratch_i, idx, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    hipLaunchKernelGGL(k_materialize, dim3((h->L.P + 255) / 256, n), dim3(256), 0, h->stream, h->bases, h->noise,
                       h->scratch_i, h->L.P, sigma, h->mat_out);
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    h->prof.materialize_ms = ms;
    if (out_host && copy_d2h(h, out_host, h->mat_out, need * sizeof(float))) return -1;
    return 0;
}

static void launch_env_reset(dne_handle *h, int n) {
    const EnvArgs E = h->env(0);
    hipLaunchKernelGGL(k_env_reset_logic, dim3((n + 63) / 64), dim3(64), 0, h->stream, E, (const uint32_t *)h->seeds, n);
    hipLaunchKernelGGL(k_env_render, dim3(n), dim3(256), 0, h->stream, E, (const int *)nullptr, 1, 1, 1);   // FrameStack reset: 4 copies
}

static void launch_env_step(dne_handle *h, const WindowPlan &w, const EnvArgs &E, const int *list, int gsize, int tslimit,
                            hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    const int items = w.cnt * gsize;
    hipLaunchKernelGGL(k_env_logic, dim3((items + 63) / 64), dim3(64), 0, st, E, list, gsize, items, tslimit);
    if (w.skip & 4) return;
    hipLaunchKernelGGL(k_env_render, dim3(items), dim3(w.render_wg), 0, st, E, list, gsize, 0, 1);
}

// ------------------------------------------------------------------------------- env ABI
static int check_n(dne_handle *h, int n) {
    if (n <= 0 || n > h->M) return h->fail("n = %d outside [1, max_members = %d]", n, h->M);
    return 0;
}

extern "C" int dne_env_reset(dne_handle *h, int n, const uint32_t *seeds) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_env_reset");
    if (check_n(h, n)) return -1;
    HCHECK(h, hipMemcpyAsync(h->seeds, seeds, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    launch_env_reset(h, n);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int dne_env_step(dne_handle *h, int n, const int32_t *actions, float *reward, int32_t *done) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_env_step");
    if (check_n(h, n)) return -1;
    for (int i = 0; i < n; i++)
        if (actions[i] < 0 || actions[i] >= h->cfg.n_actions) return h->fail("action %d out of range", actions[i]);
    HCHECK(h, hipMemcpyAsync(h->action, actions, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemsetAsync(h->step_reward, 0, n * sizeof(float), h->stream));
    launch_env_step(h, act_window(h->k, h->facts(), n), h->env(0), nullptr, 1, 0x7fffffff);
    HCHECK(h, hipGetLastError());
    if (reward) HCHECK(h, hipMemcpyAsync(reward, h->step_reward, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (done) HCHECK(h, hipMemcpyAsync(done, h->done, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int dne_env_observation(dne_handle *h, int n, uint8_t *out) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_env_observation");
    if (check_n(h, n)) return -1;
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, h->stacks, (size_t)n * OB_BYTES, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dne_env_ram(dne_handle *h, int n, uint8_t *out) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_env_ram");
    if (check_n(h, n)) return -1;
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, h->ram_cur, (size_t)n * 128, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dne_env_set_observation(dne_handle *h, int n, const uint8_t *obs) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_env_set_observation");
    if (check_n(h, n)) return -1;
    HCHECK(h, hipMemcpy(h->stacks, obs, (size_t)n * OB_BYTES, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int dne_env_set_ram(dne_handle *h, int n, const uint8_t *ram_prev, const uint8_t *ram_cur) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_env_set_ram");
    if (check_n(h, n)) return -1;
    HCHECK(h, hipMemcpyAsync(h->ram_prev, ram_prev, (size_t)n * 128, hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->ram_cur, ram_cur, (size_t)n * 128, hipMemcpyHostToDevice, h->stream));
    std::vector<int32_t> ones(n, 1);
    HCHECK(h, hipMemcpyAsync(h->stepped, ones.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    const EnvArgs E = h->env(0);
    hipLaunchKernelGGL(k_env_render, dim3(n), dim3(256), 0, h->stream, E, (const int *)nullptr, 1, 1, 1);   // fill: 4 copies
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ------------------------------------------------------------------------------- forward
extern "C" int dne_set_members(dne_handle *h, int n, const int32_t *slot, const int64_t *off, const float *scale) {
    DeviceGuard dg(h);
    if (check_n(h, n)) return -1;
    for (int i = 0; i < n; i++) {
        if (slot[i] < 0 || slot[i] >= h->base_cap) return h->fail("member %d: base slot %d not allocated", i, slot[i]);
        if (check_noise_range(h, off[i], h->L.P)) return -1;
    }
    HCHECK(h, hipMemcpyAsync(h->m_slot, slot, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->m_off, off, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->m_scale, scale, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->uniform_base = true;
    for (int i = 0; i < n; i++) h->uniform_base = h->uniform_base && slot[i] == slot[0];
    h->dense_scale = 1.0;
    h->antithetic_slot0 = h->uniform_base && slot[0] == 0 && n % 2 == 0;
    for (int i = 0; i + 1 < n && h->antithetic_slot0; i += 2)
        h->antithetic_slot0 = off[i] == off[i + 1] && scale[i] == -scale[i + 1];
    h->pair_sigma = n > 0 ? scale[0] : 0.0f;
    h->pair_sigma_uniform = h->antithetic_slot0;
    for (int i = 0; i < n && h->pair_sigma_uniform; i += 2) h->pair_sigma_uniform = scale[i] == scale[0];
    h->members_materialized = false;
    h->host_slot.assign(slot, slot + n); h->host_off.assign(off, off + n); h->host_scale.assign(scale, scale + n);
    h->host_caller.resize(n);
    for (int i = 0; i < n; i++) h->host_caller[i] = i;
    return 0;
}

// the member table as the kernels will read it (the engine's order), and whose member each row is; no kernel is launched
extern "C" int dne_debug_members(dne_handle *h, int cap, int32_t *slot, int64_t *off, float *scale, int32_t *caller_index) {
    const int n = (int)h->host_slot.size();
    for (int i = 0; i < n && i < cap; i++) {
        if (slot) slot[i] = h->host_slot[i];
        if (off) off[i] = h->host_off[i];
        if (scale) scale[i] = h->host_scale[i];
        if (caller_index) caller_index[i] = h->host_caller[i];
    }
    return n;
}

// policies.py:399: the reference batch through every member's perturbed network -> per-member BN scale/shift
static int ref_pass(dne_handle *h, int n) {
    if (!es_like(h->L.kind)) return 0;
    if (!h->ref_set) return h->fail("reference batch not set (dne_set_ref_batch)");
    const int F = h->F;
    const FwdArgs A = h->fwd(false);
    // chunks alternate between two streams with their own scratch: the statistics kernels (one workgroup per
    // member, latency-bound) of one chunk run under the MFMA convolutions of the next
    const int nways = n > h->ref_chunk ? 2 : 1;
    if (nways > 1) {
        HCHECK(h, hipEventRecord(h->ev_ref[0], h->stream));
        HCHECK(h, hipStreamWaitEvent(h->sub_streams[1], h->ev_ref[0], 0));
    }
    int c = 0;
    for (int m0 = 0; m0 < n; m0 += h->ref_chunk, c++) {
        const int nc = std::min(h->ref_chunk, n - m0), w = c % nways;
        hipStream_t st = h->sub_streams[w];
        float *y1 = h->y1r[w], *y2 = h->y2r[w], *y3p = h->y3pr[w];
        float *fr1 = h->fr1[w], *fr2 = h->fr2[w];
        const int fpw = h->k.conv1_fpw >= 8 ? 8 : h->k.conv1_fpw >= 4 ? 4 : h->k.conv1_fpw >= 2 ? 2 : 1;   // F is a multiple of 8
#define C1R(FPW) hipLaunchKernelGGL(k_conv1_ref<FPW>, dim3(nc * F / FPW), dim3(256), 0, st, A, F, m0, (const uint8_t *)h->ref, y1, fr1)
#define C1S(FPW) hipLaunchKernelGGL(k_conv1_ref_shared<FPW>, dim3((nc + 7) / 8 * (F / FPW)), dim3(512), RF_FRAME * sizeof(float), st, A, F, m0, nc, (const float *)h->ref_f32, y1, fr1)
        const bool dedup = h->ref_dedup && ref_default_route(h->k, F);
        // dedup route: y1u [nc][U1p][16] and behind it y2u [nc][U2p][32] in this way's y1r (dne_set_ref_batch checked the room)
        const int U1p = h->ref_U1p, U2p = h->ref_U2p;
        float *y2u = y1 + (size_t)h->ref_chunk * U1p * 16;
        if (dedup) {
            const int spw = 32, nseg = (U1p / C1U_ROWS + spw - 1) / spw;
            hipLaunchKernelGGL(k_conv1_ref_uniq, dim3((nc + 7) / 8 * nseg), dim3(512), 0, st, A, m0, nc, (const float *)h->ref_tab1, U1p, spw, y1);
            hipLaunchKernelGGL(k_bn1_gather, dim3(nc * (F / 8)), dim3(448), 0, st, F, 8, (const int32_t *)h->ref_idx1, (const float *)y1, U1p, fr1);
        }
        else if (h->k.conv1_shared && fpw == 8 && F % 16 == 0) C1S(16);
        else if (h->k.conv1_shared && fpw == 8) C1S(8);
        else if (fpw == 8) C1R(8); else if (fpw == 4) C1R(4); else if (fpw == 2) C1R(2); else C1R(1);
#undef C1S
#undef C1R
        // the convolutions leave per-frame moments behind; scale / shift per member is a 128-term sum per channel
        hipLaunchKernelGGL((k_bn_finalize<16>), dim3((nc * 16 + 255) / 256), dim3(256), 0, st, A, m0, nc, F, (const float *)fr1, 441, 0,
                           h->L.c1b, h->L.bn1b, h->L.bn1g);
        const bool mc_fc = F == 16 || F == 32 || F == 64 || F == 128;   // fc on the matrix cores: y2 rows padded to 128 positions
        if (dedup) {
            const int spw = 16, nseg = (U2p / C2U_ROWS + spw - 1) / spw;
            hipLaunchKernelGGL(k_conv2_ref_uniq, dim3(nc * nseg), dim3(256), C2U_LDS, st, A, m0, (const int32_t *)h->ref_win, U2p, spw, (const float *)y1, U1p, y2u);
            hipLaunchKernelGGL(k_y2_expand, dim3(nc * (F / 8)), dim3(256), 0, st, A, m0, F, 8, (const int32_t *)h->ref_idx2, (const float *)y2u, U2p, y2, fr2);
        }
        else if (mc_fc)   // 16 frames per workgroup (32 / 64 measured the same: 11.46 / 11.42 / 11.50 ms per 5000 members)
            hipLaunchKernelGGL((k_conv2_ref<16, true>), dim3(nc * (F / 16)), dim3(256), 0, st, A, F, m0, (const float *)y1, y2, fr2);
        else if (F % 8 == 0 && h->k.conv2_ref_fpw == 8)
            hipLaunchKernelGGL((k_conv2_ref<8, false>), dim3(nc * (F / 8)), dim3(256), 0, st, A, F, m0, (const float *)y1, y2, fr2);
        else if (F % 4 == 0 && h->k.conv2_ref_fpw >= 4)
            hipLaunchKernelGGL((k_conv2_ref<4, false>), dim3(nc * (F / 4)), dim3(256), 0, st, A, F, m0, (const float *)y1, y2, fr2);
        else
            hipLaunchKernelGGL((k_conv2<true>), dim3(nc * F), dim3(256), 0, st, A, (const int *)nullptr, 1, F, m0,
                               (const float *)y1, y2, 1, fr2);
        hipLaunchKernelGGL((k_bn_finalize<32>), dim3((nc * 32 + 255) / 256), dim3(256), 0, st, A, m0, nc, F, (const float *)fr2, 121, 32,
                           h->L.c2b, h->L.bn2b, h->L.bn2g);
        if (mc_fc) {   // matrix-core path
            const int grid = (nc + 7) / 8 * 8 * 4;   // (member, quarter) workgroups, those of a member on one XCD
#define FCREF(MT, NG) hipLaunchKernelGGL((k_fc_ref<MT>), dim3(grid * NG), dim3(256), MT == 4 ? FCREF4_LDS : 0, st, A, nc, m0, F, (const float *)y2, y3p)
            if (F == 16) FCREF(1, 1); else if (F == 32) FCREF(2, 1); else if (F == 64) FCREF(4, 1); else FCREF(4, 2);   // 128 frames: two groups of 64
#undef FCREF
            hipLaunchKernelGGL(k_bn3_partials, dim3(nc), dim3(256), 0, st, A, m0, F, (const float *)y3p);
        } else {
            const int nfg = F / 8;   // generic path: y3 rows live in the partial buffer of this way
            hipLaunchKernelGGL((k_fc<8, true, true, 4>), dim3((nc + 7) / 8 * 8 * nfg), dim3(256), 0, st, A,
                               (const int *)nullptr, nc, F, m0, (const float *)y2, y3p, (int32_t *)nullptr,
                               (float *)nullptr);
            hipLaunchKernelGGL(k_bn3_rows, dim3(nc), dim3(256), 0, st, A, m0, F, (const float *)y3p);
        }
    }
    if (nways > 1) {
        HCHECK(h, hipEventRecord(h->ev_ref[1], h->sub_streams[1]));
        HCHECK(h, hipStreamWaitEvent(h->stream, h->ev_ref[1], 0));
    }
    HCHECK(h, hipGetLastError());
    return 0;
}

// profiling build (-DDNE_PHASE_CLOCK): the milestones of the last launches, [6 kernels][128 workgroups][8]; -1 in the product library
extern "C" int dne_debug_phase_clock(dne_handle *h, long long *out) {
#ifdef DNE_PHASE_CLOCK
    HCHECK(h, hipDeviceSynchronize());
    HCHECK(h, hipMemcpyFromSymbol(out, HIP_SYMBOL(dne::g_phase), sizeof(long long) * 6 * 128 * 8));
    return 0;
#else
    (void)out;
    return h->fail("dne_debug_phase_clock: this library was built without DNE_PHASE_CLOCK (make clock)");
#endif
}

// profiling build: the per-workgroup records of the lock-step's kernels (env_synth.h: g_wgclk), oldest overwritten; returns the number
// of records ever written through *count (the ring holds the last min(count, cap)); reset = 1 clears the cursor afterwards
extern "C" int dne_debug_wg_clock(dne_handle *h, long long *out, unsigned cap, unsigned *count, int reset) {
#ifdef DNE_PHASE_CLOCK
    HCHECK(h, hipDeviceSynchronize());
    unsigned n = 0;
    HCHECK(h, hipMemcpyFromSymbol(&n, HIP_SYMBOL(dne::g_wgclk_n), sizeof(n)));
    if (count) *count = n;
    if (out) HCHECK(h, hipMemcpyFromSymbol(out, HIP_SYMBOL(dne::g_wgclk), sizeof(long long) * 4 * std::min(cap, dne::WGCLK_CAP)));
    if (reset) { n = 0; HCHECK(h, hipMemcpyToSymbol(HIP_SYMBOL(dne::g_wgclk_n), &n, sizeof(n))); }
    return 0;
#else
    (void)out; (void)cap; (void)count; (void)reset;
    return h->fail("dne_debug_wg_clock: this library was built without DNE_PHASE_CLOCK (make clock)");
#endif
}

// profiling build: k_fc_duo's tick stamps of its last launch (env_synth.h: g_duo_tick [64][8][288][2], g_duo_plan [64][8][8])
extern "C" int dne_debug_duo_ticks(dne_handle *h, long long *ticks, long long *plan) {
#ifdef DNE_PHASE_CLOCK
    HCHECK(h, hipDeviceSynchronize());
    HCHECK(h, hipMemcpyFromSymbol(ticks, HIP_SYMBOL(dne::g_duo_tick), sizeof(long long) * dne::DUO_TICK_WGS * 8 * dne::DUO_TICK_MAX * 2));
    HCHECK(h, hipMemcpyFromSymbol(plan, HIP_SYMBOL(dne::g_duo_plan), sizeof(long long) * dne::DUO_TICK_WGS * 8 * 8));
    return 0;
#else
    (void)ticks; (void)plan;
    return h->fail("dne_debug_duo_ticks: this library was built without DNE_PHASE_CLOCK (make clock)");
#endif
}

extern "C" int dne_ref_pass(dne_handle *h, int n) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_ref_pass");
    if (check_n(h, n)) return -1;
    if (!es_like(h->L.kind)) return h->fail("dne_ref_pass: GAAtariPolicy has no reference batch");
    if (ref_pass(h, n)) return -1;
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int dne_get_bn(dne_handle *h, int n, float *out) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_get_bn");
    if (check_n(h, n)) return -1;
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, h->bn, (size_t)n * 608 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// the batch moments of the last reference pass (tf.contrib.layers.batch_norm with decay = 0 leaves exactly these in
// moving_mean / moving_variance, policies.py:322-328): [n][608] = mean1[16] var1[16] mean2[32] var2[32] mean3[256] var3[256]
extern "C" int dne_get_bn_moments(dne_handle *h, int n, float *out) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_get_bn_moments");
    if (check_n(h, n)) return -1;
    if (!es_like(h->L.kind)) return h->fail("dne_get_bn_moments: GAAtariPolicy has no batch norm");
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, h->bn_mom, (size_t)n * 608 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// one policy decision for the groups in `list` (w.cnt groups of gsize members)
// (p, w, tt: the burst's plan, the window's and the tail table inside an evaluation; the empty plan and no table everywhere else)
static void launch_forward(dne_handle *h, const StepPlan &p, const WindowPlan &w, const TailTable *tt, const int *list, int gsize, bool use_done,
                           hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    const FwdArgs A = h->fwd(use_done, p, tt);
    const int count = w.cnt, items = count * gsize;
    const bool es = es_like(h->L.kind);
    float *y1 = use_done ? nullptr : h->y1;   // the fused kernels: dne_act / debug_activations want y1; evaluations do not
    switch (w.conv) {
    case DNE_CONV_LARGE: {   // LargeModel: three matrix-core convolutions (forward_large.h), one member at a time (GA children, or the two of an ES pair)
        constexpr size_t l2 = lconv_mfma_lds_bytes<32, 4, 2, 11, 34>(), l3 = lconv_mfma_lds_bytes<64, 3, 1, 11, 68>();
        hipLaunchKernelGGL(k_lconv1, dim3(items * 2), dim3(256), 0, st, A, list, gsize, (const uint8_t *)h->stacks, h->y1);
        const int ns = w.s2;
        with_bool(!h->members_materialized, [&](auto NOISE) {
            hipLaunchKernelGGL((k_lconv_mfma<32, 64, 4, 2, 21, 11, 1, 34, NOISE()>), dim3(items * ns), dim3(256), l2, st, A, list, gsize, A.L.c2w, A.L.c2b, (const float *)h->y1, h->y2, ns);
            hipLaunchKernelGGL((k_lconv_mfma<64, 64, 3, 1, 11, 11, 1, 68, NOISE()>), dim3(items * ns), dim3(256), l3, st, A, list, gsize, A.L.c3w, A.L.c3b, (const float *)h->y2, h->y3, ns);
        });
        return;
    }
    case DNE_CONV_FUSED:   // one workgroup per member through both convolutions, y1 stays in LDS
        with_bool(es, [&](auto ES) { hipLaunchKernelGGL((k_conv12<ES()>), dim3(items), dim3(256), sizeof(Conv12Lds), st, A, list, gsize, (const uint8_t *)h->stacks, y1, h->y2, w.act2 ? 1 : 0); });
        return;
    case DNE_CONV_TAIL4:   // the tail: four workgroups per member through both convolutions, no y1 round trip
        with_bool(es, [&](auto ES) { hipLaunchKernelGGL((k_conv12t<ES()>), dim3(items * 4), dim3(512), sizeof(Conv12Lds), st, A, list, gsize, (const uint8_t *)h->stacks, y1, h->y2); });
        break;
    default:
        if (!(w.skip & 1))
            hipLaunchKernelGGL(k_conv1, dim3(items * w.s1), dim3(256), 0, st, A, list, gsize, 1, 0,
                               (const uint8_t *)h->stacks, (const uint8_t *)nullptr, h->y1, w.s1);
        if (w.skip & 2) return;
        with_bool(es, [&](auto ES) { hipLaunchKernelGGL((k_conv2<ES()>), dim3(items * w.s2), dim3(256), 0, st, A, list, gsize, 1, 0, (const float *)h->y1, h->y2, w.s2, (float *)nullptr); });
    }
    if (w.act2) hipLaunchKernelGGL(k_y2_activate, dim3(items), dim3(256), 0, st, A, list, gsize, h->y2);
}

// k_out behind a streaming fc: the action loops unrolled over 18 where the policy has no more actions, dynamic LDS = the staged output
// weights or the caller's reservation (DNE_OUT_LDS_KB: bounds the kernel's workgroups per CU), whichever is larger
template <int NV, bool BN>
static void launch_out(hipStream_t st, int count, size_t reserve, const FwdArgs &A, const int *list, const float *sums, float *y3, int32_t *action, float *logits) {
    const size_t lds = std::max(out_stage_bytes(NV, A.L.nact), reserve);
    if (A.L.nact <= OUT_NA_ATARI) hipLaunchKernelGGL((k_out<NV, BN, OUT_NA_ATARI>), dim3(count), dim3(256), lds, st, A, list, sums, y3, action, logits);
    else hipLaunchKernelGGL((k_out<NV, BN, OUT_NA>), dim3(count), dim3(256), lds, st, A, list, sums, y3, action, logits);
}

// Test hook: k_out on inputs the caller lays out, at every width the kernel is built for (1 .. 32: dne_create admits 2 .. 18, the
// fixture's emulator has 18 actions) and under any LDS reservation.  kind: DNE_KIND_ES (batch norm, `bn` rows) or DNE_KIND_GA; gsize 2
// runs k_out<2, ..> on pairs (members 2g, 2g + 1 share off[2g]), gsize 1 k_out<1, ..>.  list NULL: groups 0 .. n_groups - 1.  y3 /
// actions / logits go in and come back, so the caller sees what the kernel left alone.  Returns 0, -1 on a refused argument or a HIP error.
extern "C" int dne_debug_out_head(int kind, int gsize, int n_actions, int n_members, const int32_t *list, int n_groups, const float *noise,
                                  size_t noise_count, const float *base, const int64_t *off, const float *scale, const int32_t *done,
                                  const float *bn, const float *sums, int sub_sums, int reserve_lds_kb, float *y3, int32_t *actions, float *logits) {
    if ((kind != DNE_KIND_ES && kind != DNE_KIND_GA) || (gsize != 1 && gsize != 2) || n_actions < 1 || n_actions > OUT_NA || n_members < gsize ||
        n_members % gsize || n_groups < 1 || reserve_lds_kb < 0 || reserve_lds_kb > 64 || !noise || !base || !off || !scale || !sums || !y3 || !actions ||
        (kind == DNE_KIND_ES && !bn))
        return -1;
    Layout L;
    make_layout(kind, n_actions, &L);
    for (int m = 0; m < n_members; m++)
        if (off[m] < 0 || (size_t)off[m] + (size_t)L.P > noise_count || off[m] != off[m - m % gsize]) return -1;
    for (int g = 0; list && g < n_groups; g++)
        if (list[g] < 0 || list[g] >= n_members / gsize) return -1;
    if (!list && n_groups > n_members / gsize) return -1;
    const size_t nsum = (size_t)n_members * (sub_sums ? 32 : 4) * 256, nlog = logits ? (size_t)n_members * n_actions : 0;
    DevBuf<float> d_noise, d_base, d_scale, d_bn, d_sums, d_y3, d_logits;
    DevBuf<int32_t> d_list, d_slot, d_done, d_act;
    DevBuf<int64_t> d_off;
#define UP(buf, src, n) do { if (buf.alloc(n) != hipSuccess || hipMemcpy(buf.p, src, (n) * sizeof(*buf.p), hipMemcpyHostToDevice) != hipSuccess) return -1; } while (0)
    UP(d_noise, noise, noise_count); UP(d_base, base, (size_t)L.P); UP(d_scale, scale, (size_t)n_members); UP(d_off, off, (size_t)n_members);
    UP(d_sums, sums, nsum); UP(d_y3, y3, (size_t)n_members * 256); UP(d_act, actions, (size_t)n_members);
    if (bn) UP(d_bn, bn, (size_t)n_members * 608);
    if (done) UP(d_done, done, (size_t)n_members);
    if (list) UP(d_list, list, (size_t)n_groups);
    if (logits) UP(d_logits, logits, nlog);
#undef UP
    if (d_slot.alloc(n_members) != hipSuccess || hipMemset(d_slot.p, 0, (size_t)n_members * sizeof(int32_t)) != hipSuccess) return -1;
    const void *outs[] = {(const void *)k_out<1, false, OUT_NA_ATARI>, (const void *)k_out<1, true, OUT_NA_ATARI>, (const void *)k_out<2, false, OUT_NA_ATARI>,
                          (const void *)k_out<2, true, OUT_NA_ATARI>,  (const void *)k_out<1, false, OUT_NA>,      (const void *)k_out<1, true, OUT_NA>,
                          (const void *)k_out<2, false, OUT_NA>,       (const void *)k_out<2, true, OUT_NA>};
    for (const void *f : outs)
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max(out_stage_bytes(2, OUT_NA), (size_t)64 * 1024)) != hipSuccess) return -1;
    FwdArgs A = {};
    A.noise = d_noise; A.bases = d_base; A.base_stride = (size_t)L.P; A.m_slot = d_slot; A.m_off = d_off; A.m_scale = d_scale; A.bn = d_bn;
    A.done = done ? d_done.p : nullptr; A.sub_sums = sub_sums ? 1 : 0; A.L = L;
    with_bool(gsize == 2, [&](auto PAIRS) { with_bool(kind == DNE_KIND_ES, [&](auto BN) {
        launch_out<PAIRS() ? 2 : 1, BN()>(nullptr, n_groups, (size_t)reserve_lds_kb * 1024, A, list ? d_list.p : nullptr, d_sums, d_y3, d_act, logits ? d_logits.p : nullptr);
    }); });
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpy(y3, d_y3, (size_t)n_members * 256 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(actions, d_act, (size_t)n_members * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (logits && hipMemcpy(logits, d_logits, nlog * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}

// the window's fc (w.fc) and, unless the caller runs k_tail_step behind it (w.head_fused), the output layer
static void launch_fc(dne_handle *h, const StepPlan &p, const WindowPlan &w, const TailTable *tt, const int *list, int gsize, float *logits,
                      hipStream_t st = nullptr,
                      const int *order = nullptr /* the window's units in noise-table order (k_unit_order), duo regime only */,
                      hipEvent_t after_stream_kernel = nullptr /* duo regime: recorded between k_fc_duo and k_out (profiling) */) {
    if (!st) st = h->stream;
    // inside an evaluation (no logits requested) groups whose members are all done are skipped: they stay in the list until
    // the next compaction, and streaming their weights would be wasted bandwidth
    const FwdArgs A = h->fwd(logits == nullptr, p, tt);
    const Knobs &k = h->k;
    const bool es = es_like(h->L.kind), out_fused = w.head_fused;
    const int count = w.cnt;
    switch (w.fc) {
    case DNE_FC_LFC_COLS: case DNE_FC_LFC: case DNE_FC_LFC_PAIR: {   // LargeModel: streamed 7744 x 512 fc (two 256-column halves per member), then relu + output layer + argmax
        const int members = count * gsize;
        const dim3 lg(std::min(2 * members, 2 * k.fc_grid));
        if (w.fc == DNE_FC_LFC_COLS) {   // few members: eight workgroups each
            with_bool(!h->members_materialized, [&](auto NOISE) { hipLaunchKernelGGL((k_lfc_cols<NOISE()>), dim3(8 * members), dim3(256), 0, st, A, list, gsize, (const float *)h->y3, h->y3t); });
        } else if (w.fc == DNE_FC_LFC_PAIR) {   // antithetic pairs over base slot 0 (plan_window): work item = (pair, half), the pair's rows fetched once
            const dim3 pg(std::min(2 * count, 2 * k.fc_grid));
            with_bool(k.fc_rb == 8, [&](auto RB8) { hipLaunchKernelGGL((k_lfc_pair<RB8() ? 8 : 4>), pg, dim3(256), 0, st, A, list, 2 * count, (const float *)h->y3, h->y3t); });
        } else if (h->members_materialized) {
            if (k.fc_rb == 8 && k.lfc_pad == 1) hipLaunchKernelGGL((k_lfc<false, 8, 1>), lg, dim3(256), 0, st, A, list, gsize, 2 * members, (const float *)h->y3, h->y3t);
            else if (k.fc_rb == 8 && k.lfc_pad == 2) hipLaunchKernelGGL((k_lfc<false, 8, 2>), lg, dim3(256), 0, st, A, list, gsize, 2 * members, (const float *)h->y3, h->y3t);
            else if (k.fc_rb == 8) hipLaunchKernelGGL((k_lfc<false, 8>), lg, dim3(256), 0, st, A, list, gsize, 2 * members, (const float *)h->y3, h->y3t);
            else hipLaunchKernelGGL((k_lfc<false, 4>), lg, dim3(256), 0, st, A, list, gsize, 2 * members, (const float *)h->y3, h->y3t);
        } else hipLaunchKernelGGL((k_lfc<true, 4>), lg, dim3(256), 0, st, A, list, gsize, 2 * members, (const float *)h->y3, h->y3t);
        hipLaunchKernelGGL(k_lout, dim3(members), dim3(256), 0, st, A, list, gsize, (const float *)h->y3t, h->action, logits);
        return;
    }
    case DNE_FC_SUB:   // mid range: one wave per sub-slice chain, folded by the head.  plan_step admits exactly two populations: ES pairs and GA children written out
        with_bool(es, [&](auto ES) {
            constexpr int NV = ES() ? 2 : 1;
            hipLaunchKernelGGL((k_fc_sub<NV, ES(), ES()>), dim3(w.sub_blocks), dim3(256), 0, st, A, list, count, w.sub_spw, k.fc_sub_prio, (const float *)h->y2, h->y3s);
            if (out_fused) return;   // the caller runs k_tail_step (FwdArgs::sub_sums tells it to fold the chain sums)
            launch_out<NV, ES()>(st, count, 0, A, list, (const float *)h->y3s, h->y3, h->action, nullptr);
        });
        return;
    case DNE_FC_QUAD: case DNE_FC_TAIL: case DNE_FC_COLS:   // latency-bound regime: 64 / 16 / 4 workgroups per group + a separate output-layer kernel
        with_bool(gsize == 2, [&](auto PAIRS) { with_bool(es, [&](auto ES) {
            constexpr int NV = PAIRS() ? 2 : 1;
            constexpr bool BN = ES();
            if (NV == 1 && !BN && h->members_materialized) {   // GA children written out: plain rows, no noise stream
                if (w.fc == DNE_FC_QUAD) hipLaunchKernelGGL((k_fc_quad<1, false, false>), dim3(count * 64), dim3(256), 0, st, A, list, (const float *)h->y2, h->y3t);
                else hipLaunchKernelGGL((k_fc_tail<1, false, false>), dim3(count * 16), dim3(512), 0, st, A, list, (const float *)h->y2, h->y3t);
            } else if (w.fc == DNE_FC_QUAD) hipLaunchKernelGGL((k_fc_quad<NV, BN>), dim3(count * 64), dim3(256), 0, st, A, list, (const float *)h->y2, h->y3t);
            else if (w.fc == DNE_FC_TAIL) hipLaunchKernelGGL((k_fc_tail<NV, BN>), dim3(count * 16), dim3(512), 0, st, A, list, (const float *)h->y2, h->y3t);
            else hipLaunchKernelGGL((k_fc_cols<NV, BN>), dim3(count * 4), dim3(256), 0, st, A, list, (const float *)h->y2, h->y3t);
            if (!out_fused) launch_out<NV, BN>(st, count, 0, A, list, (const float *)h->y3t, h->y3, h->action, logits);
        }); });
        return;
    case DNE_FC_RING: case DNE_FC_DUO: {   // table-ordered units: adjacent (pair, k-slice) units share their noise rows (ES pairs only: plan_step)
        const bool solo = w.solo;
        const int duo_grid = k.duo_grid ? k.duo_grid : k.fc_grid;
        const int n_units = 4 * count, items = ((solo ? n_units : (n_units + 1) / 2) + 3) / 4, blocks = std::min(items, duo_grid);
        const size_t out_lds = (size_t)k.out_lds_kb * 1024;   // an LDS reservation beyond k_out's own need: it only bounds the kernel's workgroups per CU next to the streaming fc
        const int flags = k.duo_lag | (solo ? 256 : 0) | (k.fc_prio << 9) | ((k.duo_sync - 1) << 11);
        if (w.fc == DNE_FC_RING) {   // one unit per wave, eight units per workgroup whatever the regime
            const int ring_blocks = std::min((n_units + 7) / 8, duo_grid);
            const float *table = w.ring_scaled ? h->noise_pre : A.noise;
            with_bool(w.ring_scaled, [&](auto PRE) { hipLaunchKernelGGL((k_fc_ring<PRE(), 8>), dim3(ring_blocks), dim3(576), 0, st, A, order, n_units, (const float *)h->y2, h->y3t, (const float *)h->theta_perm, k.fc_prio << 9, table); });
        }
        else if (w.sweep && w.fat) hipLaunchKernelGGL((k_fc_duo<2, true, true, 8, true>), dim3(blocks), dim3(256), 0, st, A, order, n_units, (const float *)h->y2, h->y3t, flags);
        else if (w.sweep) hipLaunchKernelGGL((k_fc_duo<2, true, true>), dim3(blocks), dim3(256), 0, st, A, order, n_units, (const float *)h->y2, h->y3t, flags);
        else hipLaunchKernelGGL((k_fc_duo<2, true>), dim3(blocks), dim3(256), 0, st, A, order, n_units, (const float *)h->y2, h->y3t, flags);
        if (after_stream_kernel) hipEventRecord(after_stream_kernel, st);
        if (out_fused) return;   // the caller runs k_tail_step: policy head + emulator step in one launch
        launch_out<2, true>(st, count, out_lds, A, list, (const float *)h->y3t, h->y3, h->action, nullptr);
        return;
    }
    case DNE_FC_FC2: {   // two pairs per work item share the base rows (ES pairs over one base slot only: plan_step)
        const int items = (count + 1) / 2, blocks = std::min(items, k.fc_grid);
        with_bool(k.fc_rb == 2, [&](auto RB2) { hipLaunchKernelGGL((k_fc2<true, RB2() ? 2 : 4>), dim3(blocks), dim3(256), 0, st, A, list, count, (const float *)h->y2, h->y3, h->action); });
        return;
    }
    default: {   // DNE_FC_FC
        const int fc_blocks = std::min(count, k.fc_grid);   // persistent grid (an even groups-per-block split measured slower)
        if (gsize == 1 && !es && h->members_materialized) {   // GA children written out once per generation: plain rows, no noise stream
            with_bool(k.fc_rb == 8, [&](auto RB8) { hipLaunchKernelGGL((k_fc<1, false, false, RB8() ? 8 : 4, false>), dim3(fc_blocks), dim3(256), 0, st, A, list, count, 1, 0, (const float *)h->y2, h->y3, h->action, logits); });
            return;
        }
        with_bool(gsize == 2, [&](auto PAIRS) { with_bool(es, [&](auto ES) {
            auto fc = [&](auto RB) { hipLaunchKernelGGL((k_fc<PAIRS() ? 2 : 1, false, ES(), RB()>), dim3(fc_blocks), dim3(256), 0, st, A, list, count, 1, 0, (const float *)h->y2, h->y3, h->action, logits); };
            if (k.fc_rb == 2) fc(int_c<2>{}); else if (k.fc_rb == 8) fc(int_c<8>{}); else fc(int_c<4>{});
        }); });
    }
    }
}

extern "C" int dne_act(dne_handle *h, int n, int32_t *actions, float *logits) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_act");
    if (check_n(h, n)) return -1;
    const WindowPlan w = act_window(h->k, h->facts(), n);
    launch_forward(h, StepPlan{}, w, nullptr, nullptr, 1, false);
    launch_fc(h, StepPlan{}, w, nullptr, nullptr, 1, h->logits);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (actions) HCHECK(h, hipMemcpy(actions, h->action, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (logits) HCHECK(h, hipMemcpy(logits, h->logits, (size_t)n * h->cfg.n_actions * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dne_debug_activations(dne_handle *h, int member, float *y1, float *y2, float *y3) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_debug_activations");
    if (member < 0 || member >= h->M) return h->fail("bad member");
    if (h->large) return h->fail("dne_debug_activations: LargeModel engines use dne_debug_activations_large");
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (y1) HCHECK(h, hipMemcpy(y1, h->y1 + (size_t)member * 7056, 7056 * sizeof(float), hipMemcpyDeviceToHost));
    if (y2) HCHECK(h, hipMemcpy(y2, h->y2 + (size_t)member * 3872, 3872 * sizeof(float), hipMemcpyDeviceToHost));
    if (y3) HCHECK(h, hipMemcpy(y3, h->y3 + (size_t)member * 256, 256 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// LargeModel: raw (bias added, pre-relu) outputs of conv1 [441][32], conv2 / conv3 [121][64] and the fc [512] after dne_act
extern "C" int dne_debug_activations_large(dne_handle *h, int member, float *y1, float *y2, float *y3, float *y4) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_debug_activations_large");
    if (member < 0 || member >= h->M) return h->fail("bad member");
    if (!h->large) return h->fail("dne_debug_activations_large needs a DNE_KIND_GA_LARGE engine");
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (y1) HCHECK(h, hipMemcpy(y1, h->y1 + (size_t)member * 14112, 14112 * sizeof(float), hipMemcpyDeviceToHost));
    if (y2) HCHECK(h, hipMemcpy(y2, h->y2 + (size_t)member * 7744, 7744 * sizeof(float), hipMemcpyDeviceToHost));
    if (y3) HCHECK(h, hipMemcpy(y3, h->y3 + (size_t)member * 7744, 7744 * sizeof(float), hipMemcpyDeviceToHost));
    if (y4) HCHECK(h, hipMemcpy(y4, h->y3t + (size_t)member * 512, 512 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------- batch evaluation
// tail table: with at most TT_MAX members left, all in one window, the member descriptors ride in the kernel arguments.
// Fills *tt from the active groups in list order (host_list null = 0, 1, 2, ...) and returns it, or null when no table is in force.
static const TailTable *make_tail_table(const dne_handle *h, TailTable *tt, const int *host_list, int total, int gsize, int n) {
    if (!tail_table_allowed(h->k, h->facts(), total, gsize) || total * gsize > TT_MAX || (int)h->host_off.size() < n) return nullptr;
    tt->n = total * gsize;
    for (int i = 0; i < total; i++)
        for (int v = 0; v < gsize; v++) {
            const int m = (host_list ? host_list[i] : i) * gsize + v, k = i * gsize + v;
            tt->member[k] = m; tt->slot[k] = h->host_slot[m]; tt->scale[k] = h->host_scale[m]; tt->off[k] = h->host_off[m];
        }
    return tt;
}

// the ring's DMA source: the table scaled by this evaluation's sigma (k_fc_ring<true>), made once per (table, sigma)
static int ring_scaled_table(dne_handle *h) {
    if (!h->k.ring_pre || !h->pair_sigma_uniform || h->noise_pre_no_room) return 0;
    if (!h->noise_pre && h->alloc(&h->noise_pre, h->noise_count + OVERFETCH_FLOATS, "noise_pre")) {
        h->trace("no room for the scaled table: the ring scales its rows itself");
        (void)hipGetLastError(); h->noise_pre = nullptr; h->noise_pre_no_room = true;
        return 0;
    }
    if (h->noise_pre_count != h->noise_count || h->noise_pre_sigma != h->pair_sigma) {
        static_assert(OVERFETCH_FLOATS % 4 == 0, "k_scale_table moves 16 bytes per step");
        const size_t n4 = (h->noise_count + OVERFETCH_FLOATS) / 4;   // (a table whose count is not a multiple of four leaves its last 1-3 padding floats unscaled: zeros either way)
        hipLaunchKernelGGL(k_scale_table, dim3(256 * 8), dim3(256), 0, h->stream, (const float *)h->noise, h->noise_pre, n4, h->pair_sigma);
        HCHECK(h, hipStreamSynchronize(h->stream));   // the windows' streams start behind the host
        h->noise_pre_count = h->noise_count; h->noise_pre_sigma = h->pair_sigma;
        h->trace("noise table scaled by %g for the ring", (double)h->pair_sigma);
    }
    return 0;
}

// speculative tail: the emulator + renderer outcome of every action, inside the launches of this step's forward pass
// fresh: no conv1 candidates from the previous lock-step (a new burst = a new list); next_conv1: the choice + conv1 of every candidate (not in a burst's last lock-step)
static void launch_spec_tail(dne_handle *h, const StepPlan &p, const TailTable *tt, const EnvArgs &E, const int *lst, int cnt, int gsize, int tslimit, hipStream_t sst, bool fresh, bool next_conv1) {
    const int items = cnt * gsize, nact = h->cfg.n_actions, nb = h->k.spec_bands;
    const FwdArgs A = h->fwd(true, p, tt);
    const int emu_blocks = (items * nact + 255) / 256;
    with_bool(es_like(h->L.kind), [&](auto ES) {
        if (fresh) {
            hipLaunchKernelGGL(k_conv1_spec, dim3(items * 7 + emu_blocks), dim3(256), 0, sst, A, E, lst, gsize, h->y1, 7, items * 7, items, nact);
            hipLaunchKernelGGL((k_conv2<ES()>), dim3(items * 4), dim3(256), 0, sst, A, lst, gsize, 1, 0, (const float *)h->y1, h->y2, 4, (float *)nullptr);
        } else hipLaunchKernelGGL((k_conv2_spec<ES()>), dim3(items * 4 + emu_blocks), dim3(256), 0, sst, A, E, lst, gsize, (const float *)h->y1, h->y2, 4, items * 4, items, nact, (const int32_t *)h->action);
        with_bool(gsize == 2, [&](auto PAIRS) { hipLaunchKernelGGL((k_fc_quad_spec<PAIRS() ? 2 : 1, ES()>), dim3(cnt * 64 + items * nact * nb), dim3(256), 0, sst, A, E, lst, gsize, (const float *)h->y2, h->y3t, cnt * 64, nact, nb); });
        if (next_conv1) hipLaunchKernelGGL((k_tail_select_conv1<ES()>), dim3(items + items * nact * 7), dim3(256), 0, sst, A, E, lst, gsize, tslimit, (const float *)h->y3t, h->y3, h->action, items, nact, 7);
        else hipLaunchKernelGGL((k_tail_select<ES()>), dim3(items), dim3(256), 0, sst, A, E, lst, gsize, tslimit, (const float *)h->y3t, h->y3, h->action);
    });
}

// behind an fc that left partial sums (w.head_fused): policy head + emulator step in one launch (k_tail_step), and the frames.
// w.tail: few members left -- each frame over w.render_bands workgroups, or (one band) rendered by that same launch; else behind k_fc_duo / k_fc_sub
static void launch_head_step(dne_handle *h, const StepPlan &p, const WindowPlan &w, const TailTable *tt, const EnvArgs &E, const int *lst, int gsize, int tslimit, hipStream_t sst) {
    const FwdArgs A = h->fwd(false, p, tt);
    const int items = w.cnt * gsize, nb = w.render_bands;
    const float *sums = p.sub ? h->y3s : h->y3t;
    with_bool(es_like(h->L.kind), [&](auto ES) { with_bool(w.render_fused, [&](auto R) { hipLaunchKernelGGL((k_tail_step<ES(), R()>), dim3(items), dim3(R() ? 1024 : h->k.head_threads), 0, sst, A, E, lst, gsize, tslimit, sums, h->y3, h->action); }); });
    if (w.render_fused) return;   // head + emulator + renderer in one launch
    if (w.tail) hipLaunchKernelGGL(k_env_render, dim3(items * nb), dim3(w.render_wg), 0, sst, E, lst, gsize, 0, nb);
    else if (!(w.skip & 4)) hipLaunchKernelGGL(k_env_render, dim3(items), dim3(w.render_wg), 0, sst, E, lst, gsize, 0, 1);
}

// profiling engines: one step counter per bracketed launch set, zeroed
static int reserve_launch_units(dne_handle *h, int tslimit) {
    const size_t need = (size_t)h->sub_streams.size() * (size_t)tslimit + 64;
    if (need > h->launch_units_cap) {
        HCHECK(h, h->release(h->launch_units));
        HCHECK(h, h->alloc(&h->launch_units, need, "launch_units"));
        h->launch_units_cap = need;
    }
    HCHECK(h, hipMemsetAsync(h->launch_units, 0, need * sizeof(int32_t), h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// the event pool of a profiled evaluation into dne_profile (evs: per bracketed launch set {before, after conv, after fc, after env})
static int reduce_profile(dne_handle *h, const std::vector<std::array<size_t, 4>> &evs) {
    dne_profile &P = h->prof;
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_pool[0], h->ev_pool[1]));
    P.ref_ms = ms;
    std::vector<int32_t> units(evs.size());
    if (!evs.empty()) HCHECK(h, hipMemcpy(units.data(), h->launch_units, evs.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<std::pair<float, float>> iv;   // fc intervals relative to the start of the reference pass
    for (size_t i = 0; i < evs.size(); i++) {
        const auto &e = evs[i];
        HCHECK(h, hipEventElapsedTime(&ms, h->ev_pool[e[0]], h->ev_pool[e[1]])); P.conv_ms += ms;
        HCHECK(h, hipEventElapsedTime(&ms, h->ev_pool[e[1]], h->ev_pool[e[2]])); P.fc_ms += ms;
        P.fc_full_ms += ms; P.fc_full_launches += 1; P.fc_full_units += units[i];
        float t0 = 0;
        HCHECK(h, hipEventElapsedTime(&t0, h->ev_pool[0], h->ev_pool[e[1]]));
        iv.push_back({t0, t0 + ms});
        HCHECK(h, hipEventElapsedTime(&ms, h->ev_pool[e[2]], h->ev_pool[e[3]])); P.env_ms += ms;
    }
    std::sort(iv.begin(), iv.end());
    double uni = 0; float hi = -1;
    for (auto &p : iv) {   // length of the union of the intervals
        if (p.first > hi) { uni += p.second - p.first; hi = p.second; }
        else if (p.second > hi) { uni += p.second - hi; hi = p.second; }
    }
    P.fc_full_union_ms = uni;
    return 0;
}

// policies.py:378-429 / 473-513 for n members at once: reset, (ES) reference pass, then lock-step
// act -> env.step over the shrinking list of active groups until every episode is done.
static int eval_core(dne_handle *h, int n, int gsize, int tslimit, const uint32_t *env_seed, float *returns,
                     float *signreturns, int32_t *lengths, uint8_t *bc_out) {
    if (n % gsize) return h->fail("member count %d not a multiple of the group size %d", n, gsize);
    if (tslimit <= 0) return h->fail("timestep limit must be positive");
    if (bc_out && !h->bc) return h->fail("behaviour characterisations requested but the engine was created with record_bc = 0");
    const bool prof = h->cfg.profile_events != 0;
    // record_bc engines always record (the trajectories feed dne_novelty_batch on the device); bc_out only controls the download
    const int bc_mode = h->bc ? (es_like(h->L.kind) && !h->cfg.bc_final_only ? 1 : 2) : 0;
    // rows past an episode's length are never read on the device (dne_novelty_batch takes the lengths); zero them only
    // when the whole buffer is about to be downloaded
    if (bc_mode == 1 && bc_out) HCHECK(h, hipMemsetAsync(h->bc, 0, (size_t)n * h->cfg.bc_max_steps * 128, h->stream));
    if (bc_mode == 2) HCHECK(h, hipMemsetAsync(h->bc, 0, (size_t)n * 128, h->stream));
    h->ram_last_n = 0;   // (set again at the end: an evaluation that fails half way leaves no points to score)
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    HCHECK(h, hipMemcpyAsync(h->seeds, env_seed, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    launch_env_reset(h, n);
    if (prof) HCHECK(h, hipEventRecord(h->event(0), h->stream));
    h->trace("eval: %d members (groups of %d), tslimit %d: reset launched", n, gsize, tslimit);
    if (h->debug_sync) { HCHECK(h, hipStreamSynchronize(h->stream)); HCHECK(h, hipGetLastError()); }
    if (h->theta_perm && h->antithetic_slot0 && gsize == 2)   // k_fc_ring reads base slot 0's fc matrix in its own column order
        hipLaunchKernelGGL(k_theta_perm, dim3(3872 + 16), dim3(256), 0, h->stream, (const float *)(h->bases + h->L.fcw), h->theta_perm, 3872);
    if (ref_pass(h, n)) return -1;
    if (h->debug_sync) { HCHECK(h, hipDeviceSynchronize()); HCHECK(h, hipGetLastError()); }
    h->trace("eval: reference pass %s", h->debug_sync ? "done" : "launched");
    HCHECK(h, hipEventRecord(h->event(1), h->stream));
    const int groups = n / gsize;
    hipLaunchKernelGGL(k_iota, dim3((groups + 255) / 256), dim3(256), 0, h->stream, h->list_a, groups);
    HCHECK(h, hipStreamSynchronize(h->stream));

    int *cur = h->list_a, *nxt = h->list_b;
    int total = groups;
    TailTable tt_store;
    const TailTable *tt = make_tail_table(h, &tt_store, nullptr, total, gsize, n);
    EnvArgs E = h->env(bc_mode, tt);
    int t = 0;
    long long group_steps = 0, launch_sets = 0;
    std::vector<std::array<size_t, 4>> evs;   // per profiled launch set: event indices {before, after conv, after fc, after env}
    size_t ne = 2;
    if (prof && reserve_launch_units(h, tslimit)) return -1;
    hipEvent_t last_fc = nullptr;
    size_t fc_ring_pos = 0;
    // the evaluation as a whole, by the width it starts with: its profiled ("full") launches are one kernel, one roofline line (plan.h: window_profiled)
    const StepPlan ev = plan_step(h->k, h->facts(), groups, gsize, true);
    if (ev.ring && ring_scaled_table(h)) return -1;
    const PlanFacts facts = h->facts();   // (behind ring_scaled_table: nothing changes them before the evaluation ends)
    while (total > 0 && t < tslimit) {
        const int burst = std::min(burst_length(h->k, total), tslimit - t);   // lock-steps until the next compaction
        const StepPlan p = plan_step(h->k, facts, total, gsize);
        const int nsub = p.nsub;   // windows of this burst
        std::array<WindowPlan, N_STREAMS> win;
        for (int s = 0; s < nsub; s++) {
            const Window c = window(total, nsub, s);
            win[s] = plan_window(h->k, facts, p, total, c.cnt, gsize, true);
            win[s].lo = c.lo;
            if (is_duo(win[s]))   // the list only changes at a compaction: rank each window's units by table address once per burst
                hipLaunchKernelGGL(k_unit_order, dim3((4 * c.cnt + 255) / 256), dim3(256), (size_t)4 * c.cnt * sizeof(long long), h->sub_streams[s],
                                   (const int64_t *)h->m_off, (const int *)(cur + c.lo), c.cnt, gsize, h->unit_order + 4 * c.lo);
        }
        for (int st = 0; st < burst; st++) {
            for (int s = 0; s < nsub; s++) {
                const WindowPlan &w = win[s];
                const int lo = w.lo, cnt = w.cnt;
                if (cnt == 0) continue;
                hipStream_t sst = h->sub_streams[s];
                const int *lst = cur + lo;
                std::array<size_t, 4> e{};
                const bool pe = prof && window_profiled(ev, p, w);   // events only around full-width launches
                if (pe) { e[0] = ne++; HCHECK(h, hipEventRecord(h->event(e[0]), sst)); }
                if (w.spec) launch_spec_tail(h, p, tt, E, lst, cnt, gsize, tslimit, sst, st == 0 || !h->k.spec_conv1, h->k.spec_conv1 && st + 1 < burst);
                else {
                    launch_forward(h, p, w, tt, lst, gsize, true, sst);
                    if (w.chain && last_fc) HCHECK(h, hipStreamWaitEvent(sst, last_fc, 0));
                    if (pe) { e[1] = ne++; HCHECK(h, hipEventRecord(h->event(e[1]), sst)); }   // after the wait: brackets fc only
                    if (pe) e[2] = ne++;
                    launch_fc(h, p, w, tt, lst, gsize, nullptr, sst, is_duo(w) ? h->unit_order + 4 * lo : nullptr,
                              pe && is_duo(w) ? h->event(e[2]) : nullptr);   // duo: the bracket ends behind k_fc_duo, before k_out
                    if (w.chain) { last_fc = h->fc_ring[fc_ring_pos++ % h->fc_ring.size()]; HCHECK(h, hipEventRecord(last_fc, sst)); }
                    if (pe && !is_duo(w)) HCHECK(h, hipEventRecord(h->event(e[2]), sst));
                    E.step_counter = pe ? h->launch_units + evs.size() : nullptr;
                    if (w.head_fused) launch_head_step(h, p, w, tt, E, lst, gsize, tslimit, sst);
                    else launch_env_step(h, w, E, lst, gsize, tslimit, sst);
                    if (pe) { e[3] = ne++; HCHECK(h, hipEventRecord(h->event(e[3]), sst)); evs.push_back(e); }
                }
                if (h->debug_sync) {
                    hipError_t de = hipStreamSynchronize(sst);
                    if (de == hipSuccess) de = hipGetLastError();
                    if (de != hipSuccess && w.spec) return h->fail("lock-step %d (speculative tail, %d active groups): %s", t + st, cnt, hipGetErrorString(de));
                    if (de != hipSuccess) return h->fail("lock-step %d window %d/%d (%d of %d active groups, %s): %s", t + st, s, nsub, cnt, total, fc_name(w.fc), hipGetErrorString(de));
                }
                group_steps += cnt;
                launch_sets++;
            }
        }
        t += burst;
        for (int s = 1; s < nsub; s++) HCHECK(h, hipStreamSynchronize(h->sub_streams[s]));
        hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, h->stream, (const int32_t *)h->done, gsize, (const int *)cur,
                           total, nxt, h->count_dev);
        HCHECK(h, hipMemcpyAsync(h->count_host, h->count_dev, (8 + TT_MAX) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HCHECK(h, hipStreamSynchronize(h->stream));
        total = *h->count_host;
        std::swap(cur, nxt);
        tt = make_tail_table(h, &tt_store, h->count_host + 8, total, gsize, n);
        set_tail_table(E, tt);
        h->trace("eval: lock-step %d, %d active groups", t, total);
    }
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipMemcpyAsync(returns, h->ret, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (signreturns) HCHECK(h, hipMemcpyAsync(signreturns, h->sign, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipMemcpyAsync(lengths, h->len, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (bc_out && copy_d2h(h, bc_out, h->bc, bc_mode == 1 ? (size_t)n * h->cfg.bc_max_steps * 128 : (size_t)n * 128)) return -1;
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    dne_profile &P = h->prof;
    P.eval_ms = ms;
    P.fc_ms = P.conv_ms = P.env_ms = P.ref_ms = 0;
    P.fc_launches = launch_sets;
    P.fc_group_steps = group_steps;
    P.env_steps = 0;
    for (int i = 0; i < n; i++) P.env_steps += lengths[i];
    P.fc_full_ms = P.fc_full_launches = P.fc_full_units = 0;
    P.fc_full_kind = fc_full_kind(ev);
    P.fc_full_union_ms = 0;
    if (prof && reduce_profile(h, evs)) return -1;
    if (bc_mode == 2) {   // dne_ram_novelty_pool(bc = NULL) / dne_archive_append_members: row j of bc is the caller's member ram_last_caller[j] --
        h->ram_last_n = n;   // j itself for a caller of this function's own entry points; ga_eval_impl, which reorders its members, says otherwise
        h->ram_last_caller.resize(n);
        for (int j = 0; j < n; j++) h->ram_last_caller[j] = j;
    }
    return 0;
}


// ------------------------------------------------------------------------------- the hard maze (csrc/maze.h)
static int maze_check(std::string *err, const float *header8, const float *lines, int n_walls) {
    if (!header8 || !lines) { *err = "maze: header or lines missing"; return -1; }
    if (n_walls < 1 || n_walls > maze::MAX_WALLS) { *err = "maze: " + std::to_string(n_walls) + " walls, the kernel and the host function take 1.." + std::to_string(maze::MAX_WALLS); return -1; }
    return 0;
}

static maze::Header maze_header(const float *h8) {
    maze::Header m;
    m.disable = h8[0]; m.steps = h8[1]; m.sx = h8[2]; m.sy = h8[3]; m.heading = h8[4]; m.gx = h8[5]; m.gy = h8[6]; m.reserved = h8[7];
    return m;
}

// ---- what the four whole-episode kinds share on the host: the evaluation, the arguments, the trace, the final state ----
// where a rollout's members come from: descriptors (slot, off, scale) over the rows of `bases`
struct MazeMembers { const float *bases; const int32_t *slot; const int64_t *off; const float *scale; };

// the members set by dne_set_members
static MazeMembers maze_set_members(dne_handle *h) { return {h->bases, h->m_slot, h->m_off, h->m_scale}; }

// what every k_*_rollout reads for members [first, first + count) of M; the kind's own inputs and every output are left null
template <class Args>
static Args member_args(dne_handle *h, const MazeMembers &M, int first, int count, int tslimit) {
    Args A{};
    A.noise = h->noise; A.bases = M.bases; A.base_stride = h->base_stride;
    A.m_slot = M.slot; A.m_off = M.off; A.m_scale = M.scale;
    A.first = first; A.count = count; A.tslimit = tslimit;
    return A;
}

// One evaluation of members [0, n), a whole episode each: launch() between ev_a and ev_b, the returns, sign-returns and lengths copied back, the
// profile written.  What a kind refuses, uploads or clears comes before this call; what it counts (its *_last_n) after a 0 from here.
template <class Launch>
static int run_episodes(dne_handle *h, int n, float *returns, float *signreturns, int32_t *lengths, Launch &&launch) {
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    launch();
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipMemcpyAsync(returns, h->ret, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (signreturns) HCHECK(h, hipMemcpyAsync(signreturns, h->sign, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipMemcpyAsync(lengths, h->len, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    dne_profile &P = h->prof;
    P = dne_profile{};
    P.eval_ms = P.env_ms = ms;
    P.fc_launches = 1;
    for (int i = 0; i < n; i++) P.env_steps += lengths[i];
    return 0;
}

// what dne_{cartpole,pendulum,mjmaze}_debug_trace ask first ...
static int trace_args(dne_handle *h, const char *call, int kind, int member, bool args_ok) {
    if (needs_kind(h, call, kind)) return -1;
    if (member < 0 || member >= (int)h->host_slot.size()) return h->fail("%s: member %d, dne_set_members set %zu", call, member, h->host_slot.size());
    return args_ok ? 0 : h->fail("%s: bad arguments", call);
}

// ... and do last: launch(trace rows, step count) for one block, then the rows the kernel says it wrote, cap at the most
template <class T, class Launch>
static int run_trace(dne_handle *h, const char *call, int cap, int width, T *trace, int32_t *steps, Launch &&launch) {
    DevBuf<T> d;
    DevBuf<int32_t> dn;
    HCHECK(h, d.alloc((size_t)cap * width));
    HCHECK(h, dn.alloc(1));
    launch((T *)d, (int32_t *)dn);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(steps, dn, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*steps < 0 || *steps > cap) return h->fail("%s: the kernel reports %d steps under a limit of %d", call, *steps, cap);
    HCHECK(h, hipMemcpy(trace, d, (size_t)*steps * width * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// rows [0, n) of a per-member buffer of the last evaluation (its final states: `width` values a member)
template <class T>
static int last_eval_rows(dne_handle *h, const char *call, int n, int last_n, bool out_ok, T *out, const T *dev, int width) {
    if (n < 1 || n > last_n) return h->fail("%s: %d members asked for, the last evaluation ran %d", call, n, last_n);
    if (!out_ok) return h->fail("%s: no output buffer", call);
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, dev, (size_t)n * width * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// the calls DNE_KIND_MJMAZE shares with DNE_KIND_MAZE: the walls, the final positions, the archive and dne_maze_novelty
static int needs_maze_env(dne_handle *h, const char *call) {
    return h->mjmaze ? 0 : needs_kind(h, call, DNE_KIND_MAZE);   // (every other kind: the refusal it always got)
}

extern "C" int dne_maze_set_walls(dne_handle *h, const float *header8, const float *lines, int n) {
    DeviceGuard dg(h);
    if (!(h->dense && h->dn_shape.env == DNE_KIND_MAZE) && needs_maze_env(h, "dne_maze_set_walls")) return -1;   // (a dense policy on the maze shares the walls)
    if (maze_check(&h->err, header8, lines, n)) return -1;
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(h->maze_walls, lines, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice));
    h->maze_hdr = maze_header(header8);
    h->maze_nw = n;
    return 0;
}

// what k_maze_rollout reads for members [first, first + count) of M; its outputs are left null (maze_eval_members and the trace set theirs)
static maze::RolloutArgs maze_args(dne_handle *h, const MazeMembers &M, int first, int count, int tslimit) {
    maze::RolloutArgs A = member_args<maze::RolloutArgs>(h, M, first, count, tslimit);
    A.hdr = h->maze_hdr; A.walls = h->maze_walls; A.nw = h->maze_nw;
    return A;
}

// members [0, n) of M (dne_set_members', or the GA bank's), one whole episode each, one launch
static int maze_eval_members(dne_handle *h, const MazeMembers &M, int n, int tslimit, float *returns, float *signreturns, int32_t *lengths, uint8_t *bc_out) {
    if (h->maze_nw < 1) return h->fail("DNE_KIND_MAZE: no maze loaded (dne_maze_set_walls comes before an evaluation)");
    if (tslimit <= 0) return h->fail("timestep limit must be positive");
    if (bc_out && !h->bc) return h->fail("behaviour characterisations requested but the engine was created with record_bc = 0");
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    const size_t bc_floats = (size_t)n * std::max(h->cfg.bc_max_steps, 1) * 2;
    if (h->bc && bc_out) HCHECK(h, hipMemsetAsync(h->bc, 0, bc_floats * sizeof(float), h->stream));   // rows past an episode's length read as zero
    maze::RolloutArgs A = maze_args(h, M, 0, n, tslimit);
    A.ret = h->ret; A.sign = h->sign; A.len = h->len; A.xy = h->maze_xy;
    A.bc = (float *)h->bc; A.bc_max_steps = h->bc ? std::max(h->cfg.bc_max_steps, 1) : 0;
    if (run_episodes(h, n, returns, signreturns, lengths, [&] { hipLaunchKernelGGL(maze::k_maze_rollout, dim3((n + 3) / 4), dim3(64), 0, h->stream, A); })) return -1;
    if (bc_out) HCHECK(h, hipMemcpy(bc_out, h->bc, bc_floats * sizeof(float), hipMemcpyDeviceToHost));
    h->maze_last_n = n;
    return 0;
}

extern "C" int dne_maze_final_state(dne_handle *h, int n, float *xy) {
    DeviceGuard dg(h);
    if (needs_maze_env(h, "dne_maze_final_state")) return -1;
    return last_eval_rows(h, "dne_maze_final_state", n, h->maze_last_n, true /* (xy is not looked at) */, xy, (const float *)h->maze_xy, 2);
}

// the kernel once more for ONE of the current members, with every step written out: trace [min(tslimit, 400)][16] as dne_maze_rollout_host
// writes it.  The accumulators of the last evaluation are left alone.
extern "C" int dne_maze_debug_trace(dne_handle *h, int member, int tslimit, float *trace) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_maze_debug_trace", DNE_KIND_MAZE)) return -1;
    if (h->maze_nw < 1) return h->fail("DNE_KIND_MAZE: no maze loaded (dne_maze_set_walls comes before an evaluation)");
    if (member < 0 || member >= (int)h->host_slot.size()) return h->fail("dne_maze_debug_trace: member %d, dne_set_members set %zu", member, h->host_slot.size());
    if (tslimit <= 0 || !trace) return h->fail("dne_maze_debug_trace: bad arguments");
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    const int steps = std::min(tslimit, (int)maze::EPISODE_STEPS);
    DevBuf<float> d;
    HCHECK(h, d.alloc((size_t)steps * maze::TRACE_W));
    maze::RolloutArgs A = maze_args(h, maze_set_members(h), member, 1, tslimit);
    A.trace = d;
    hipLaunchKernelGGL(maze::k_maze_rollout, dim3(1), dim3(64), 0, h->stream, A);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(trace, d, (size_t)steps * maze::TRACE_W * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// the same header on the CPU: no handle, no GPU (like dne_debug_plan).  trace rows past an episode's length are not written.
extern "C" int dne_maze_rollout_host(const float *theta, int n, const float *header8, const float *lines, int n_walls, int tslimit,
                                     float *returns, int32_t *lengths, float *xy, float *trace) {
    if (maze_check(&g_create_error, header8, lines, n_walls)) return -1;
    if (n < 1 || tslimit <= 0 || !theta || !returns || !lengths || !xy) { g_create_error = "dne_maze_rollout_host: bad arguments"; return -1; }
    const maze::Header m = maze_header(header8);
    for (int i = 0; i < n; i++)
        maze::rollout_host(theta + (size_t)i * maze::NPARAMS, m, lines, n_walls, tslimit, returns + i, lengths + i, xy + 2 * i,
                           trace ? trace + (size_t)i * tslimit * maze::TRACE_W : nullptr);
    return 0;
}

// test hooks on the CPU: the environment alone under n open-loop action sequences of T steps (rows [n][T][18], obs0 [n][11] or NULL), and
// the forward pass alone for n (theta, observation) pairs (h1, h2 [n][16] after their relus, out [n][2])
extern "C" int dne_maze_actions_host(const float *actions, int n, int T, const float *header8, const float *lines, int n_walls, float *rows,
                                     float *obs0) {
    if (maze_check(&g_create_error, header8, lines, n_walls)) return -1;
    if (n < 1 || T < 1 || !actions || !rows) { g_create_error = "dne_maze_actions_host: bad arguments"; return -1; }
    const maze::Header m = maze_header(header8);
    for (int i = 0; i < n; i++)
        maze::actions_host(actions + (size_t)i * T * 2, T, m, lines, n_walls, rows + (size_t)i * T * 18, obs0 ? obs0 + (size_t)i * maze::OBS : nullptr);
    return 0;
}

extern "C" int dne_maze_forward_host(const float *theta, const float *obs, int n, float *h1, float *h2, float *out) {
    if (n < 1 || !theta || !obs || !h1 || !h2 || !out) { g_create_error = "dne_maze_forward_host: bad arguments"; return -1; }
    for (int i = 0; i < n; i++)
        maze::forward_host(theta + (size_t)i * maze::NPARAMS, obs + (size_t)i * maze::OBS, h1 + (size_t)i * maze::HID, h2 + (size_t)i * maze::HID,
                           out + (size_t)i * maze::ACT);
    return 0;
}

// the math probe (maze.h: math_probe) on the CPU and, one thread per input, on the device: out [n][2] doubles
extern "C" int dne_maze_math_host(int fn, const double *x, int n, double *out) {
    if (fn < 0 || fn >= maze::MATH_FNS || n < 1 || !x || !out) { g_create_error = "dne_maze_math_host: bad arguments (fn 0..3, n >= 1)"; return -1; }
    for (int i = 0; i < n; i++) maze::math_probe(fn, x[i], out + 2 * (size_t)i);
    return 0;
}

extern "C" int dne_maze_debug_math(dne_handle *h, int fn, const double *x, int n, double *out) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_maze_debug_math", DNE_KIND_MAZE)) return -1;
    if (fn < 0 || fn >= maze::MATH_FNS || n < 1 || !x || !out) return h->fail("dne_maze_debug_math: bad arguments (fn 0..3, n >= 1)");
    DevBuf<double> dx, dout;
    HCHECK(h, dx.alloc((size_t)n)); HCHECK(h, dout.alloc(2 * (size_t)n));
    HCHECK(h, hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(maze::k_maze_math, dim3((n + 255) / 256), dim3(256), 0, h->stream, fn, (const double *)dx, n, (double *)dout);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, dout, 2 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------- Deep-GA on the hard maze (csrc/maze_ga.h)
static float *mzg_bank(dne_handle *h, int half) { return h->mzg_mem + (size_t)half * h->M * h->base_stride; }

extern "C" int dne_maze_ga_set_init_scale(dne_handle *h, const float *scale_by, size_t n) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_maze_ga_set_init_scale", DNE_KIND_MAZE)) return -1;
    if (n != (size_t)maze_ga::P || !scale_by) return h->fail("dne_maze_ga_set_init_scale: expected %d values, got %zu", maze_ga::P, n);
    if (!h->mzg_mem) {
        const size_t M = h->M;
        HCHECK(h, h->alloc(&h->init_scale, n, "maze_ga_init_scale"));
        HCHECK(h, h->alloc(&h->mzg_slot, M, "maze_ga_slot")); HCHECK(h, h->alloc(&h->mzg_off, M, "maze_ga_off")); HCHECK(h, h->alloc(&h->mzg_scale, M, "maze_ga_scale"));
        float *mem = nullptr;
        HCHECK(h, h->alloc(&mem, 3 * M * h->base_stride, "maze_ga_bank"));
        HCHECK(h, hipMemset(mem, 0, 3 * M * h->base_stride * sizeof(float)));
        h->mzg_mem = mem;
    }
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(h->init_scale, scale_by, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// what every call that reads the table or the bank needs first
static int mzg_ready(dne_handle *h, const char *call, bool walls) {
    if (!h->mzg_mem) return h->fail("%s: no init scale (dne_maze_ga_set_init_scale comes first)", call);
    if (!h->noise) return h->fail("%s: noise table not uploaded (dne_noise_upload)", call);
    if (walls && h->maze_nw < 1) return h->fail("%s: no maze loaded (dne_maze_set_walls comes before an evaluation)", call);
    return 0;
}

static int mzg_upload_members(dne_handle *h, int n, const int32_t *a, const int64_t *b, const float *c) {
    HCHECK(h, hipMemcpyAsync(h->mzg_slot, a, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->mzg_off, b, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->mzg_scale, c, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    return 0;
}

extern "C" int dne_maze_ga_build(dne_handle *h, int T, const int32_t *chain_offsets, const int64_t *seeds, const float *powers) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_maze_ga_build", DNE_KIND_MAZE)) return -1;
    if (mzg_ready(h, "dne_maze_ga_build", false)) return -1;
    if (T < 1 || T > h->M) return h->fail("dne_maze_ga_build: T = %d outside [1, max_members = %d]", T, h->M);
    if (!chain_offsets || !seeds || !powers) return h->fail("dne_maze_ga_build: a buffer is missing");
    if (chain_offsets[0] != 0) return h->fail("dne_maze_ga_build: chain_offsets starts at %d, not 0", chain_offsets[0]);
    const std::string bad = maze_ga::check_genomes(T, chain_offsets, seeds, h->noise_count);
    if (!bad.empty()) return h->fail("dne_maze_ga_build: %s", bad.c_str());
    const size_t total = (size_t)chain_offsets[T];
    if (total > h->mzg_chain_cap || !h->mzg_chain_offs) {
        HCHECK(h, hipStreamSynchronize(h->stream));
        HCHECK(h, h->release(h->mzg_chain_offs)); HCHECK(h, h->release(h->mzg_seeds)); HCHECK(h, h->release(h->mzg_powers));
        h->mzg_chain_cap = std::max<size_t>(2 * total, 4096);
        HCHECK(h, h->alloc(&h->mzg_chain_offs, (size_t)h->M + 1, "maze_ga_chain_offs"));
        HCHECK(h, h->alloc(&h->mzg_seeds, h->mzg_chain_cap, "maze_ga_seeds")); HCHECK(h, h->alloc(&h->mzg_powers, h->mzg_chain_cap, "maze_ga_powers"));
    }
    HCHECK(h, hipMemcpyAsync(h->mzg_chain_offs, chain_offsets, ((size_t)T + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->mzg_seeds, seeds, total * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->mzg_powers, powers, total * sizeof(float), hipMemcpyHostToDevice, h->stream));
    const int other = 1 - h->mzg_half;
    hipLaunchKernelGGL(maze_ga::k_maze_ga_build, dim3(T, 2), dim3(256), 0, h->stream, (const float *)h->noise, (const float *)h->init_scale,
                       (const int32_t *)h->mzg_chain_offs, (const int64_t *)h->mzg_seeds, (const float *)h->mzg_powers, mzg_bank(h, other), h->base_stride);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));   // the caller's arrays may go away
    h->mzg_half = other; h->mzg_T = T;
    return 0;
}

extern "C" int dne_maze_ga_promote(dne_handle *h, int T_new, const int32_t *parent, const int64_t *idx, const float *power) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_maze_ga_promote", DNE_KIND_MAZE)) return -1;
    if (mzg_ready(h, "dne_maze_ga_promote", false)) return -1;
    if (T_new < 1 || T_new > h->M) return h->fail("dne_maze_ga_promote: T = %d outside [1, max_members = %d]", T_new, h->M);
    if (!parent || !idx || !power) return h->fail("dne_maze_ga_promote: a buffer is missing");
    for (int j = 0; j < T_new; j++) {
        const std::string bad = maze_ga::check_member(j, h->mzg_T, h->noise_count, parent[j], idx[j], true);
        if (!bad.empty()) return h->fail("dne_maze_ga_promote: %s", bad.c_str());
    }
    if (mzg_upload_members(h, T_new, parent, idx, power)) return -1;
    const int other = 1 - h->mzg_half;
    hipLaunchKernelGGL(maze_ga::k_maze_ga_promote, dim3(T_new, 2), dim3(256), 0, h->stream, (const float *)h->noise, (const float *)h->init_scale,
                       (const float *)mzg_bank(h, h->mzg_half), mzg_bank(h, other), h->base_stride, (const int32_t *)h->mzg_slot,
                       (const int64_t *)h->mzg_off, (const float *)h->mzg_scale);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->mzg_half = other; h->mzg_T = T_new;
    return 0;
}

extern "C" int dne_maze_ga_eval(dne_handle *h, int n, const int32_t *parent, const int64_t *idx, const float *power, int tslimit,
                                float *returns, float *signreturns, int32_t *lengths) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_maze_ga_eval", DNE_KIND_MAZE)) return -1;
    if (mzg_ready(h, "dne_maze_ga_eval", true)) return -1;
    if (n < 1 || n > h->M) return h->fail("dne_maze_ga_eval: n = %d outside [1, max_members = %d]", n, h->M);
    if (!parent || !idx || !power || !returns || !lengths) return h->fail("dne_maze_ga_eval: a buffer is missing");
    if (tslimit <= 0) return h->fail("dne_maze_ga_eval: timestep limit must be positive");
    // a child is the rollout kernel's own member: (its parent's bank slot, idx, power); a root runs from scratch slot 2 M + i at scale 0
    const int bank0 = h->mzg_half * h->M, root0 = 2 * h->M;
    std::vector<int32_t> &slot = h->mzg_host_slot;
    std::vector<float> &scale = h->mzg_host_scale;
    slot.resize(n); scale.resize(n);
    bool roots = false;
    for (int i = 0; i < n; i++) {
        const std::string bad = maze_ga::check_member(i, h->mzg_T, h->noise_count, parent[i], idx[i], false);
        if (!bad.empty()) return h->fail("dne_maze_ga_eval: %s", bad.c_str());
        const bool root = parent[i] < 0;
        slot[i] = root ? root0 + i : bank0 + parent[i];
        scale[i] = root ? 0.0f : power[i];
        roots = roots || root;
    }
    if (mzg_upload_members(h, n, slot.data(), idx, scale.data())) return -1;
    if (roots) {
        hipLaunchKernelGGL(maze_ga::k_maze_ga_roots, dim3(n, 2), dim3(256), 0, h->stream, (const float *)h->noise, (const float *)h->init_scale,
                           (const int32_t *)h->mzg_slot, (const int64_t *)h->mzg_off, root0, h->mzg_mem, h->base_stride);
        HCHECK(h, hipGetLastError());
    }
    return maze_eval_members(h, MazeMembers{h->mzg_mem, h->mzg_slot, h->mzg_off, h->mzg_scale}, n, tslimit, returns, signreturns, lengths, nullptr);
}

extern "C" int dne_maze_ga_parents(dne_handle *h) {
    if (needs_kind(h, "dne_maze_ga_parents", DNE_KIND_MAZE)) return -1;
    return h->mzg_T;
}

extern "C" int dne_maze_ga_get_parent(dne_handle *h, int j, float *out) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_maze_ga_get_parent", DNE_KIND_MAZE)) return -1;
    if (j < 0 || j >= h->mzg_T) return h->fail("dne_maze_ga_get_parent: parent %d, the bank holds %d", j, h->mzg_T);
    if (!out) return h->fail("dne_maze_ga_get_parent: no output buffer");
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, mzg_bank(h, h->mzg_half) + (size_t)j * h->base_stride, maze_ga::P * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// the same header on the CPU: no handle, no GPU
static int mzg_host_table(const char *call, const float *noise, size_t count, const float *scale_by) {
    if (!noise || !scale_by) { g_create_error = std::string(call) + ": a buffer is missing"; return -1; }
    if (count < (size_t)maze_ga::P) { g_create_error = std::string(call) + ": a table of " + std::to_string(count) + " floats holds no 498 parameters"; return -1; }
    return 0;
}

extern "C" int dne_maze_ga_theta_host(const float *noise, size_t count, const float *scale_by, const int64_t *seeds, const float *powers, int nseeds,
                                      float *out) {
    if (mzg_host_table("dne_maze_ga_theta_host", noise, count, scale_by)) return -1;
    if (!seeds || !powers || !out) { g_create_error = "dne_maze_ga_theta_host: a buffer is missing"; return -1; }
    const int32_t co[2] = {0, nseeds};
    const std::string bad = maze_ga::check_genomes(1, co, seeds, count);
    if (!bad.empty()) { g_create_error = "dne_maze_ga_theta_host: " + bad; return -1; }
    maze_ga::genome_host(noise, scale_by, seeds, powers, nseeds, out);
    return 0;
}

extern "C" int dne_maze_ga_members_host(const float *noise, size_t count, const float *scale_by, const float *bank, int T, const int32_t *parent,
                                        const int64_t *idx, const float *power, int n, float *out) {
    if (mzg_host_table("dne_maze_ga_members_host", noise, count, scale_by)) return -1;
    if (n < 1) { g_create_error = "dne_maze_ga_members_host: n = " + std::to_string(n) + ", at least one member is needed"; return -1; }
    if (T < 0 || (T > 0 && !bank)) { g_create_error = "dne_maze_ga_members_host: T = " + std::to_string(T) + " parents without a bank"; return -1; }
    if (!parent || !idx || !power || !out) { g_create_error = "dne_maze_ga_members_host: a buffer is missing"; return -1; }
    for (int i = 0; i < n; i++) {
        const std::string bad = maze_ga::check_member(i, T, count, parent[i], idx[i], true);
        if (!bad.empty()) { g_create_error = "dne_maze_ga_members_host: " + bad; return -1; }
    }
    maze_ga::members_host(noise, scale_by, bank, parent, idx, power, n, out);
    return 0;
}

// ------------------------------------------------------------------------------- novelty on the hard maze (csrc/maze_novelty.h)
constexpr size_t MZN_ARCH_CAP0 = 64;   // points of the archive's first allocation; it doubles from there

// the buffer holds at least `need` elements afterwards; the first `keep` survive a reallocation (copied on the engine's stream)
template <typename T>
static int mzn_reserve(dne_handle *h, T *&p, size_t &cap, size_t need, size_t keep, size_t floor, const char *name) {
    if (need <= cap) return 0;
    const size_t ncap = std::max(std::max(2 * cap, need), floor);
    T *q = nullptr;
    HCHECK(h, h->alloc(&q, ncap, name));
    if (p && keep) HCHECK(h, hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));   // whatever still reads or fills the old buffer has finished
    HCHECK(h, h->release(p));
    p = q; cap = ncap;
    return 0;
}

// xy == NULL: the last evaluation's members where k_maze_rollout left them
static int mzn_check_members(dne_handle *h, const char *call, const float *xy, int n) {
    if (n < 1) return h->fail("%s: n = %d, at least one point is needed", call, n);
    if (!xy && n > h->maze_last_n) return h->fail("%s: %d members asked for, the last evaluation ran %d", call, n, h->maze_last_n);
    return 0;
}

// room behind the archive's points for `more` of them; the points already there survive a reallocation
static int mzn_archive_room(dne_handle *h, const char *call, int more) {
    const size_t have = (size_t)h->mzn_arch_n;
    if (have + (size_t)more > (size_t)INT_MAX / 2) return h->fail("%s: %zu points would not fit an int", call, have + (size_t)more);
    return mzn_reserve(h, h->mzn_arch, h->mzn_arch_cap, 2 * (have + more), 2 * have, 2 * MZN_ARCH_CAP0, "maze_archive");
}

extern "C" int dne_maze_archive_append(dne_handle *h, const float *xy, int n) {
    DeviceGuard dg(h);
    if (needs_maze_env(h, "dne_maze_archive_append")) return -1;
    if (mzn_check_members(h, "dne_maze_archive_append", xy, n)) return -1;
    if (mzn_archive_room(h, "dne_maze_archive_append", n)) return -1;
    const size_t have = (size_t)h->mzn_arch_n;
    if (xy) {
        HCHECK(h, hipMemcpyAsync(h->mzn_arch + 2 * have, xy, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HCHECK(h, hipStreamSynchronize(h->stream));   // the caller's buffer is free again
    } else {
        HCHECK(h, hipMemcpyAsync(h->mzn_arch + 2 * have, h->maze_xy, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    h->mzn_arch_n += n;
    return 0;
}

extern "C" int dne_maze_archive_clear(dne_handle *h) {
    DeviceGuard dg(h);
    if (needs_maze_env(h, "dne_maze_archive_clear")) return -1;
    h->mzn_arch_n = 0;   // (the buffer stays; a later append lands behind every call already on the stream)
    return 0;
}

extern "C" int dne_maze_archive_size(dne_handle *h) {
    if (needs_maze_env(h, "dne_maze_archive_size")) return -1;
    return h->mzn_arch_n;
}

extern "C" int dne_maze_archive_get(dne_handle *h, float *xy, int cap) {
    DeviceGuard dg(h);
    if (needs_maze_env(h, "dne_maze_archive_get")) return -1;
    if (cap < h->mzn_arch_n) return h->fail("dne_maze_archive_get: room for %d points, the archive holds %d", cap, h->mzn_arch_n);
    if (h->mzn_arch_n > 0) {
        if (!xy) return h->fail("dne_maze_archive_get: no buffer");
        HCHECK(h, hipMemcpyAsync(xy, h->mzn_arch, (size_t)h->mzn_arch_n * 2 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HCHECK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

// what both scoring calls refuse alike, before the refusals of their own
static int mzn_score_args(dne_handle *h, const char *call, bool pool, const float *xy, int n, int k) {
    if (pool ? needs_kind(h, call, DNE_KIND_MAZE) : needs_maze_env(h, call)) return -1;   // (pool novelty is GA-NS's: DNE_KIND_MAZE only)
    if (mzn_check_members(h, call, xy, n)) return -1;
    if (k < 1) return h->fail("%s: k = %d, at least one neighbour is needed", call, k);
    if (k > DNE_MAZE_NOVELTY_KMAX) return h->fail("%s: k = %d, the kernel keeps at most DNE_MAZE_NOVELTY_KMAX = %d neighbours", call, k, DNE_MAZE_NOVELTY_KMAX);
    return 0;
}

// ... and what both do behind them: xy staged (or the last evaluation's positions), the form's kernel over the kk <= k nearest between two
// events, the n novelties back
static int mzn_score(dne_handle *h, const char *call, bool pool, const float *xy, int n, int kk, double *out) {
    if (!out) return h->fail("%s: no output buffer", call);
    const float *pts = h->maze_xy;
    if (xy) {
        if (mzn_reserve(h, h->mzn_xy, h->mzn_xy_cap, 2 * (size_t)n, 0, 4096, "maze_novelty_xy")) return -1;
        HCHECK(h, hipMemcpyAsync(h->mzn_xy, xy, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        pts = h->mzn_xy;
    }
    if (mzn_reserve(h, h->mzn_out, h->mzn_out_cap, (size_t)n, 0, 4096, "maze_novelty_out")) return -1;
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    hipLaunchKernelGGL((pool ? maze_novelty::k_maze_novelty_pool : maze_novelty::k_maze_novelty), dim3((n + 3) / 4), dim3(256), 0, h->stream, pts, n,
                       (const float *)h->mzn_arch, h->mzn_arch_n, kk, h->mzn_out);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipMemcpyAsync(out, h->mzn_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    h->mzn_last_ms = ms;
    return 0;
}

extern "C" int dne_maze_novelty(dne_handle *h, const float *xy, int n, int k, double *out) {
    DeviceGuard dg(h);
    if (mzn_score_args(h, "dne_maze_novelty", false, xy, n, k)) return -1;
    if (h->mzn_arch_n < 1) return h->fail("dne_maze_novelty: the archive is empty (dne_maze_archive_append)");
    return mzn_score(h, "dne_maze_novelty", false, xy, n, std::min(k, h->mzn_arch_n), out);
}

// pool novelty (GA-NS): every member against the archive and the other members
extern "C" int dne_maze_novelty_pool(dne_handle *h, const float *xy, int n, int k, double *out) {
    DeviceGuard dg(h);
    if (mzn_score_args(h, "dne_maze_novelty_pool", true, xy, n, k)) return -1;
    if (h->mzn_arch_n + (n - 1) < 1) return h->fail("dne_maze_novelty_pool: the pool is empty (one member, no archive point)");
    if ((size_t)h->mzn_arch_n + (size_t)n > (size_t)INT_MAX / 2) return h->fail("dne_maze_novelty_pool: %zu combined slots would not fit an int", (size_t)h->mzn_arch_n + (size_t)n);
    return mzn_score(h, "dne_maze_novelty_pool", true, xy, n, std::min(k, h->mzn_arch_n + n - 1), out);
}

// archive slot A + i = the final position of the last evaluation's member members[i], device to device (k_maze_archive_gather)
extern "C" int dne_maze_archive_append_members(dne_handle *h, const int32_t *members, int count) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_maze_archive_append_members", DNE_KIND_MAZE)) return -1;
    if (count < 1) return h->fail("dne_maze_archive_append_members: count = %d, at least one member is needed", count);
    if (!members) return h->fail("dne_maze_archive_append_members: no member indices");
    for (int i = 0; i < count; i++)
        if (members[i] < 0 || members[i] >= h->maze_last_n)
            return h->fail("dne_maze_archive_append_members: index %d is member %d, the last evaluation ran %d", i, members[i], h->maze_last_n);
    if (mzn_archive_room(h, "dne_maze_archive_append_members", count)) return -1;
    const size_t have = (size_t)h->mzn_arch_n;
    if (mzn_reserve(h, h->mzn_idx, h->mzn_idx_cap, (size_t)count, 0, 4096, "maze_archive_members")) return -1;
    HCHECK(h, hipMemcpyAsync(h->mzn_idx, members, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(maze_novelty::k_maze_archive_gather, dim3((count + 255) / 256), dim3(256), 0, h->stream, (const float *)h->maze_xy,
                       (const int32_t *)h->mzn_idx, count, h->mzn_arch + 2 * have);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));   // the caller's buffer is free again
    h->mzn_arch_n += count;
    return 0;
}

extern "C" double dne_maze_novelty_last_ms(dne_handle *h) { return h->mzn_last_ms; }

// the same header on the CPU: no handle, no GPU
extern "C" int dne_maze_novelty_host(const float *xy, int n, const float *archive, int narch, int k, double *out) {
    if (!xy || !archive || !out) { g_create_error = "dne_maze_novelty_host: a buffer is missing"; return -1; }
    if (n < 1) { g_create_error = "dne_maze_novelty_host: n = " + std::to_string(n) + ", at least one point is needed"; return -1; }
    if (narch < 1) { g_create_error = "dne_maze_novelty_host: the archive is empty"; return -1; }
    if (k < 1) { g_create_error = "dne_maze_novelty_host: k = " + std::to_string(k) + ", at least one neighbour is needed"; return -1; }
    maze_novelty::novelty_host(xy, n, archive, narch, k, out);
    return 0;
}

extern "C" int dne_maze_novelty_pool_host(const float *xy, int n, const float *archive, int narch, int k, double *out) {
    if (!xy || !out || (narch > 0 && !archive)) { g_create_error = "dne_maze_novelty_pool_host: a buffer is missing"; return -1; }
    if (n < 1) { g_create_error = "dne_maze_novelty_pool_host: n = " + std::to_string(n) + ", at least one point is needed"; return -1; }
    if (narch < 0) { g_create_error = "dne_maze_novelty_pool_host: narch = " + std::to_string(narch); return -1; }
    if (k < 1) { g_create_error = "dne_maze_novelty_pool_host: k = " + std::to_string(k) + ", at least one neighbour is needed"; return -1; }
    if ((long long)narch + n - 1 < 1) { g_create_error = "dne_maze_novelty_pool_host: the pool is empty (one member, no archive point)"; return -1; }
    maze_novelty::novelty_pool_host(xy, n, archive, narch, k, out);
    return 0;
}

// ------------------------------------------------------------------------------- gym.CartPole-v1 (csrc/cartpole.h)
// what k_cartpole_rollout reads for the members [first, first + count) set by dne_set_members; its outputs are left null
static cartpole::RolloutArgs cartpole_args(dne_handle *h, int first, int count, int tslimit) {
    cartpole::RolloutArgs A = member_args<cartpole::RolloutArgs>(h, maze_set_members(h), first, count, tslimit);
    A.seed = h->seeds;
    return A;
}

// members [0, n), one whole episode each under its own reset seed, one launch
static int cartpole_eval(dne_handle *h, const char *call, int n, int tslimit, const uint32_t *env_seed, float *returns, float *signreturns,
                         int32_t *lengths, uint8_t *bc_out) {
    if (bc_out) return h->fail("%s: behaviour characterisations are not available on a DNE_KIND_CARTPOLE engine (kind %d): bc must be NULL; "
                               "dne_cartpole_final_state has the final state of every member", call, DNE_KIND_CARTPOLE);
    if (tslimit <= 0) return h->fail("timestep limit must be positive");
    if (!env_seed) return h->fail("%s: a DNE_KIND_CARTPOLE engine resets every member from its environment seed, env_seed is NULL", call);
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    HCHECK(h, hipMemcpyAsync(h->seeds, env_seed, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    cartpole::RolloutArgs A = cartpole_args(h, 0, n, tslimit);
    A.ret = h->ret; A.sign = h->sign; A.len = h->len; A.state = h->cp_state;
    if (run_episodes(h, n, returns, signreturns, lengths, [&] { hipLaunchKernelGGL(cartpole::k_cartpole_rollout, dim3((n + 3) / 4), dim3(64), 0, h->stream, A); })) return -1;
    h->cp_last_n = n;
    return 0;
}

extern "C" int dne_cartpole_final_state(dne_handle *h, int n, double *state) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_cartpole_final_state", DNE_KIND_CARTPOLE)) return -1;
    return last_eval_rows(h, "dne_cartpole_final_state", n, h->cp_last_n, state != nullptr, state, (const double *)h->cp_state, 4);
}

// the kernel once more for ONE of the current members, with every step written out: trace [min(tslimit, 500)][8] as
// dne_cartpole_rollout_host writes it.  The accumulators of the last evaluation are left alone.
extern "C" int dne_cartpole_debug_trace(dne_handle *h, int member, int tslimit, const double *init4, double *trace, int32_t *steps) {
    DeviceGuard dg(h);
    if (trace_args(h, "dne_cartpole_debug_trace", DNE_KIND_CARTPOLE, member, tslimit > 0 && trace && steps)) return -1;
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    cartpole::RolloutArgs A = cartpole_args(h, member, 1, tslimit);
    if (init4) { A.has_init = 1; for (int i = 0; i < 4; i++) A.init4[i] = init4[i]; }
    return run_trace(h, "dne_cartpole_debug_trace", std::min(tslimit, (int)cartpole::EPISODE_STEPS), cartpole::TRACE_W, trace, steps, [&](double *rows, int32_t *count) {
        A.trace = rows; A.trace_steps = count;
        hipLaunchKernelGGL(cartpole::k_cartpole_rollout, dim3(1), dim3(64), 0, h->stream, A);
    });
}

// the same header on the CPU: no handle, no GPU (like dne_maze_rollout_host)
extern "C" int dne_cartpole_reset_host(uint32_t seed, double *out4) {
    if (!out4) { g_create_error = "dne_cartpole_reset_host: no output buffer"; return -1; }
    const cartpole::State s = cartpole::reset_state(seed);
    out4[0] = s.x; out4[1] = s.x_dot; out4[2] = s.theta; out4[3] = s.theta_dot;
    return 0;
}

extern "C" int dne_cartpole_rollout_host(const float *theta, int n, const uint32_t *seeds, const double *init4, int tslimit, float *returns,
                                         int32_t *lengths, double *state, double *trace) {
    if (n < 1 || tslimit <= 0 || !theta || !seeds || !returns || !lengths || !state) { g_create_error = "dne_cartpole_rollout_host: bad arguments"; return -1; }
    for (int i = 0; i < n; i++) {
        lengths[i] = cartpole::rollout_host(theta + (size_t)i * cartpole::NPARAMS, seeds[i], init4 ? init4 + 4 * (size_t)i : nullptr, tslimit,
                                            state + 4 * (size_t)i, trace ? trace + (size_t)i * tslimit * cartpole::TRACE_W : nullptr);
        returns[i] = (float)lengths[i];
    }
    return 0;
}

extern "C" int dne_cartpole_actions_host(const int32_t *actions, int n, int T, const double *init4, double *rows) {
    if (n < 1 || T < 1 || !actions || !init4 || !rows) { g_create_error = "dne_cartpole_actions_host: bad arguments"; return -1; }
    for (size_t i = 0; i < (size_t)n * T; i++)
        if (actions[i] != 0 && actions[i] != 1) { g_create_error = "dne_cartpole_actions_host: action " + std::to_string(actions[i]) + ", CartPole-v1 has actions 0 and 1"; return -1; }
    for (int i = 0; i < n; i++) cartpole::actions_host(actions + (size_t)i * T, T, init4 + 4 * (size_t)i, rows + (size_t)i * T * 5);
    return 0;
}

extern "C" int dne_cartpole_forward_host(const float *theta, const float *obs, int n, float *h1, float *h2, float *out) {
    if (n < 1 || !theta || !obs || !h1 || !h2 || !out) { g_create_error = "dne_cartpole_forward_host: bad arguments"; return -1; }
    for (int i = 0; i < n; i++)
        cartpole::forward_host(theta + (size_t)i * cartpole::NPARAMS, obs + (size_t)i * cartpole::OBS, h1 + (size_t)i * cartpole::HID,
                               h2 + (size_t)i * cartpole::HID, out + (size_t)i * cartpole::ACT);
    return 0;
}

// ------------------------------------------------------------------------------- MujocoPolicy on the pendulum (csrc/pendulum.h)
// ---- what DNE_KIND_PENDULUM and DNE_KIND_MJMAZE share on the host; a call is told which of the two it belongs to by one of these
struct MujocoKind { int kind; const char *name; int obs, ac_values; };   // (name: dne_<name>_*; the observation width; the action-noise values a member reads)
static const MujocoKind MJ_PENDULUM = {DNE_KIND_PENDULUM, "pendulum", pendulum::OBS, pendulum::EPISODE_STEPS};
static const MujocoKind MJ_MAZE = {DNE_KIND_MJMAZE, "mjmaze", mjmaze::OBS, mjmaze::AC_NOISE};

// f(int_c<H>, std::bool_constant<TANH>) for the engine's hidden width and nonlinearity: the six instantiations of a MujocoPolicy kernel
template <class F>
static void with_mujoco_shape(const dne_handle *h, F &&f) {
    const bool th = h->pd_nl == pendulum::NL_TANH;
    switch (h->pd_hidden) {
    case 64: with_bool(th, [&](auto TANH) { f(int_c<64>{}, TANH); }); break;
    case 128: with_bool(th, [&](auto TANH) { f(int_c<128>{}, TANH); }); break;
    default: with_bool(th, [&](auto TANH) { f(int_c<256>{}, TANH); });
    }
}

// "" when every member's action-noise values [off, off + values) lie inside a table of `count` values (an offset < 0: the member reads none), else
// the refusal; say_values: in the setter's words, which name how many values a member reads
static std::string ac_off_refusal(const char *call, const int64_t *off, int n, int values, size_t count, bool say_values) {
    for (int i = 0; i < n; i++)
        if (off[i] >= 0 && (uint64_t)off[i] + values > (uint64_t)count)
            return std::string(call) + ": member " + std::to_string(i) + " reads its " + (say_values ? std::to_string(values) + " action-noise values" : "action noise") +
                   " from offset " + std::to_string(off[i]) + ", past the noise table's " + std::to_string(count) + " values";
    return "";
}
static int ac_off_check(dne_handle *h, const char *call, const int64_t *off, int n, int values, bool say_values) {   // ... of a device call
    const std::string bad = ac_off_refusal(call, off, n, values, h->noise_count, say_values);
    return bad.empty() ? 0 : h->fail("%s", bad.c_str());
}
static int ac_off_check_host(const char *call, const int64_t *off, int n, int values, size_t count) {               // ... of a host call
    const std::string bad = ac_off_refusal(call, off, n, values, count, false);
    if (!bad.empty()) g_create_error = bad;
    return bad.empty() ? 0 : -1;
}

static int mujoco_shape_host(const char *call, bool ok, int hidden, int n_out, int ac_mode, int nonlin, const char *header) {
    if (!ok)
        g_create_error = std::string(call) + ": hidden width " + std::to_string(hidden) + ", " + std::to_string(n_out) + " outputs, action mode " +
                         std::to_string(ac_mode) + ", nonlinearity " + std::to_string(nonlin) + " is not a shape csrc/" + header + " builds";
    return ok ? 0 : -1;
}

static int mujoco_set_ob_stat(dne_handle *h, const MujocoKind &K, const char *call, const float *mean, const float *std) {
    DeviceGuard dg(h);
    if (needs_kind(h, call, K.kind)) return -1;
    if (!mean || !std) return h->fail("%s: bad arguments", call);
    with_mujoco_options(h, [&](auto &o) { fill_options(o, o.n_out, o.ac_mode, o.ac_noise_std, mean, std); });
    h->mo.stat_set = true;
    return 0;
}

// action noise and observation statistics of the NEXT evaluation's first n members (later members: neither); that evaluation clears them
static int mujoco_set_rollout_options(dne_handle *h, const MujocoKind &K, const char *call, int n, float ac_noise_std, const int64_t *ac_off, const uint8_t *stat_flag) {
    DeviceGuard dg(h);
    dne_handle::MujocoOptions &O = h->mo;
    if (needs_kind(h, call, K.kind)) return -1;
    if (check_n(h, n)) return -1;
    if (!h->noise && ac_off) return h->fail("noise table not uploaded (dne_noise_upload)");
    if (ac_off && ac_off_check(h, call, ac_off, n, K.ac_values, true)) return -1;
    O.has_off = ac_off != nullptr; O.has_flag = stat_flag != nullptr;
    if (ac_off) O.host_off.assign(ac_off, ac_off + n); else O.host_off.clear();
    if (ac_off) HCHECK(h, hipMemcpyAsync(O.off, ac_off, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    if (stat_flag) HCHECK(h, hipMemcpyAsync(O.flag, stat_flag, n, hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    with_mujoco_options(h, [&](auto &o) { o.ac_noise_std = ac_noise_std; });
    O.n = n;
    return 0;
}

// what an evaluation and the trace ask alike of the statistics ...
static int mujoco_stat_ready(dne_handle *h, const MujocoKind &K, const char *call) {
    return h->mo.stat_set ? 0 : h->fail("%s: the observation statistics of a %s engine are NaN until dne_%s_set_ob_stat is called", call, episodic_kind_name(K.kind), K.name);
}

// ... and what an evaluation of n members asks of the options last: they were given for n members, and the table (it may have been replaced
// since) still holds every member's action noise
static int mujoco_options_ready(dne_handle *h, const MujocoKind &K, const char *call, int n) {
    const dne_handle::MujocoOptions &O = h->mo;
    if ((O.has_off || O.has_flag) && O.n != n)
        return h->fail("%s: dne_%s_set_rollout_options was given %d members, this evaluation runs %d", call, K.name, O.n, n);
    return O.has_off ? ac_off_check(h, call, O.host_off.data(), n, K.ac_values, false) : 0;
}

// the options and the statistics buffers into an evaluation's arguments (A.opt is the handle's already); the options were for this evaluation only
template <class Args>
static void mujoco_take_options(dne_handle *h, Args &A) {
    dne_handle::MujocoOptions &O = h->mo;
    A.ac_off = O.has_off ? O.off : nullptr; A.stat_flag = O.has_flag ? O.flag : nullptr;
    A.ob_sum = O.sum; A.ob_sumsq = O.sumsq; A.ob_count = O.count;
    O.has_off = O.has_flag = false; O.n = 0;
    with_mujoco_options(h, [](auto &o) { o.ac_noise_std = 0.0f; });
}

static int mujoco_ob_stats(dne_handle *h, const MujocoKind &K, const char *call, int n, double *sum, double *sumsq, int32_t *count) {
    DeviceGuard dg(h);
    if (needs_kind(h, call, K.kind)) return -1;
    if (n < 1 || n > h->pd_last_n) return h->fail("%s: %d members asked for, the last evaluation ran %d", call, n, h->pd_last_n);
    if (!sum || !sumsq || !count) return h->fail("%s: no output buffer", call);
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(sum, h->mo.sum, (size_t)n * K.obs * sizeof(double), hipMemcpyDeviceToHost));
    HCHECK(h, hipMemcpy(sumsq, h->mo.sumsq, (size_t)n * K.obs * sizeof(double), hipMemcpyDeviceToHost));
    HCHECK(h, hipMemcpy(count, h->mo.count, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

// ---- the pendulum's own
extern "C" int dne_pendulum_num_params(int hidden, int n_out) {
    if (!pendulum::hidden_ok(hidden) || n_out < 1 || n_out > pendulum::MAX_OUT) return -1;
    return pendulum::offsets(hidden, n_out).P;
}

// what k_pendulum_rollout reads for the members [first, first + count) of M (dne_set_members', or the GA bank's); the per-member options and the
// outputs are left null
static pendulum::RolloutArgs pendulum_args(dne_handle *h, const MazeMembers &M, int first, int count, int tslimit) {
    pendulum::RolloutArgs A = member_args<pendulum::RolloutArgs>(h, M, first, count, tslimit);
    A.seed = h->seeds; A.opt = h->pd_opt;
    return A;
}

static void pendulum_launch(dne_handle *h, const pendulum::RolloutArgs &A) {
    with_mujoco_shape(h, [&](auto H, auto TANH) { hipLaunchKernelGGL((pendulum::k_pendulum_rollout<H(), TANH()>), dim3(A.count), dim3(H()), 0, h->stream, A); });
}

extern "C" int dne_pendulum_set_ob_stat(dne_handle *h, const float *mean, const float *std) {
    return mujoco_set_ob_stat(h, MJ_PENDULUM, "dne_pendulum_set_ob_stat", mean, std);
}

extern "C" int dne_pendulum_set_rollout_options(dne_handle *h, int n, float ac_noise_std, const int64_t *ac_off, const uint8_t *stat_flag) {
    return mujoco_set_rollout_options(h, MJ_PENDULUM, "dne_pendulum_set_rollout_options", n, ac_noise_std, ac_off, stat_flag);
}

// members [0, n) of M, one whole episode each under its own reset seed, one launch
static int pendulum_eval(dne_handle *h, const MazeMembers &M, const char *call, int n, int tslimit, const uint32_t *env_seed, float *returns, float *signreturns,
                         int32_t *lengths, uint8_t *bc_out) {
    if (bc_out) return h->fail("%s: behaviour characterisations are not available on a DNE_KIND_PENDULUM engine (kind %d): bc must be NULL; "
                               "dne_pendulum_final_state has the final state of every member", call, DNE_KIND_PENDULUM);
    if (tslimit <= 0) return h->fail("timestep limit must be positive");
    if (!env_seed) return h->fail("%s: a DNE_KIND_PENDULUM engine resets every member from its environment seed, env_seed is NULL", call);
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    if (mujoco_stat_ready(h, MJ_PENDULUM, call) || mujoco_options_ready(h, MJ_PENDULUM, call, n)) return -1;
    HCHECK(h, hipMemcpyAsync(h->seeds, env_seed, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    pendulum::RolloutArgs A = pendulum_args(h, M, 0, n, tslimit);
    A.ret = h->ret; A.sign = h->sign; A.len = h->len; A.state = h->pd_state;
    mujoco_take_options(h, A);
    if (run_episodes(h, n, returns, signreturns, lengths, [&] { pendulum_launch(h, A); })) return -1;
    h->pd_last_n = n;
    return 0;
}

extern "C" int dne_pendulum_ob_stats(dne_handle *h, int n, double *sum, double *sumsq, int32_t *count) {
    return mujoco_ob_stats(h, MJ_PENDULUM, "dne_pendulum_ob_stats", n, sum, sumsq, count);
}

extern "C" int dne_pendulum_final_state(dne_handle *h, int n, double *state) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_pendulum_final_state", DNE_KIND_PENDULUM)) return -1;
    return last_eval_rows(h, "dne_pendulum_final_state", n, h->pd_last_n, state != nullptr, state, (const double *)h->pd_state, 2);
}

// the kernel once more for ONE of the current members, with every step written out: trace [min(tslimit, 200)][8] as dne_pendulum_rollout_host
// writes it; no action noise, no statistics.  The accumulators of the last evaluation are left alone.
extern "C" int dne_pendulum_debug_trace(dne_handle *h, int member, int tslimit, const double *init2, double *trace, int32_t *steps) {
    DeviceGuard dg(h);
    if (trace_args(h, "dne_pendulum_debug_trace", DNE_KIND_PENDULUM, member, tslimit > 0 && trace && steps)) return -1;
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    if (mujoco_stat_ready(h, MJ_PENDULUM, "dne_pendulum_debug_trace")) return -1;
    pendulum::RolloutArgs A = pendulum_args(h, maze_set_members(h), member, 1, tslimit);
    A.opt.ac_noise_std = 0.0f;
    if (init2) { A.has_init = 1; A.init2[0] = init2[0]; A.init2[1] = init2[1]; }
    return run_trace(h, "dne_pendulum_debug_trace", std::min(tslimit, (int)pendulum::EPISODE_STEPS), pendulum::TRACE_W, trace, steps, [&](double *rows, int32_t *count) {
        A.trace = rows; A.trace_steps = count;
        pendulum_launch(h, A);
    });
}

// tanh_f, norm_angle and the normalise-and-clip of one component, value by value on the device (fn: pendulum.h's MATH_*; a, b: mean and std of fn 2)
extern "C" int dne_pendulum_debug_math(dne_handle *h, int fn, const double *x, int n, float a, float b, double *out) {
    DeviceGuard dg(h);
    if (needs_kind(h, "dne_pendulum_debug_math", DNE_KIND_PENDULUM)) return -1;
    if (fn < 0 || fn >= pendulum::MATH_FNS || n < 1 || !x || !out) return h->fail("dne_pendulum_debug_math: bad arguments");
    DevBuf<double> dx, dy;
    HCHECK(h, dx.alloc(n)); HCHECK(h, dy.alloc(n));
    HCHECK(h, hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pendulum::k_pendulum_math, dim3((n + 255) / 256), dim3(256), 0, h->stream, fn, (const double *)dx, n, a, b, (double *)dy);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, dy, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// the same header on the CPU: no handle, no GPU
extern "C" int dne_pendulum_reset_host(uint32_t seed, double *out2) {
    if (!out2) { g_create_error = "dne_pendulum_reset_host: no output buffer"; return -1; }
    const pendulum::State s = pendulum::reset_state(seed);
    out2[0] = s.theta; out2[1] = s.theta_dot;
    return 0;
}

static int pendulum_shape_host(const char *call, int hidden, int n_out, int ac_mode, int nonlin) {
    const bool ok = pendulum::hidden_ok(hidden) && (nonlin == pendulum::NL_TANH || nonlin == pendulum::NL_RELU) &&
                    (ac_mode == pendulum::AC_CONTINUOUS ? n_out == 1 : (ac_mode == pendulum::AC_UNIFORM && n_out >= 2 && n_out <= pendulum::MAX_OUT));
    return mujoco_shape_host(call, ok, hidden, n_out, ac_mode, nonlin, "pendulum.h");
}

// one episode for each of n thetas [n][P] under seeds [n] (init2 [n][2] or NULL).  table / ac_off [n] (both or neither; an offset < 0: no noise for
// that member), stat_flag [n] or NULL: as the device call's options.  Outputs as the kernel writes them; trace [n][tslimit][8] or NULL.
extern "C" int dne_pendulum_rollout_host(const float *theta, int n, int hidden, int n_out, int ac_mode, int nonlin, const float *mean, const float *std,
                                         const uint32_t *seeds, const double *init2, int tslimit, float ac_noise_std, const float *table, size_t table_len,
                                         const int64_t *ac_off, const uint8_t *stat_flag, float *returns, float *signreturns, int32_t *lengths,
                                         double *state, double *ob_sum, double *ob_sumsq, int32_t *ob_count, double *trace) {
    if (n < 1 || tslimit <= 0 || !theta || !mean || !std || !seeds || !returns || !signreturns || !lengths || !state || !ob_sum || !ob_sumsq || !ob_count ||
        (ac_off != nullptr) != (table != nullptr)) { g_create_error = "dne_pendulum_rollout_host: bad arguments"; return -1; }
    if (pendulum_shape_host("dne_pendulum_rollout_host", hidden, n_out, ac_mode, nonlin)) return -1;
    pendulum::Options o{};
    fill_options(o, n_out, ac_mode, ac_noise_std, mean, std);
    const size_t P = pendulum::offsets(hidden, n_out).P;
    if (ac_off && ac_off_check_host("dne_pendulum_rollout_host", ac_off, n, MJ_PENDULUM.ac_values, table_len)) return -1;
    for (int i = 0; i < n; i++) {
        const bool stat = stat_flag && stat_flag[i];
        const pendulum::Episode e = pendulum::rollout_host(hidden, nonlin, theta + (size_t)i * P, o, seeds[i], init2 ? init2 + 2 * (size_t)i : nullptr, tslimit,
                                                           ac_off && ac_off[i] >= 0 ? table + ac_off[i] : nullptr, stat,
                                                           trace ? trace + (size_t)i * tslimit * pendulum::TRACE_W : nullptr);
        returns[i] = e.ret; signreturns[i] = e.sign; lengths[i] = e.len;
        state[2 * (size_t)i] = e.s.theta; state[2 * (size_t)i + 1] = e.s.theta_dot;
        for (int c = 0; c < pendulum::OBS; c++) { ob_sum[3 * (size_t)i + c] = e.ob_sum[c]; ob_sumsq[3 * (size_t)i + c] = e.ob_sumsq[c]; }
        ob_count[i] = stat ? e.len : 0;
    }
    return 0;
}

extern "C" int dne_pendulum_actions_host(const float *actions, int n, int T, const double *init2, double *rows) {
    if (n < 1 || T < 1 || !actions || !init2 || !rows) { g_create_error = "dne_pendulum_actions_host: bad arguments"; return -1; }
    for (int i = 0; i < n; i++) pendulum::actions_host(actions + (size_t)i * T, T, init2 + 2 * (size_t)i, rows + (size_t)i * T * 3);
    return 0;
}

// the policy alone: thetas [n][P] on raw observations [n][3] -> x [n][3] (normalised and clipped), h1 [n][H], h2 [n][H], out [n][n_out], action [n]
extern "C" int dne_pendulum_forward_host(const float *theta, const float *obs, int n, int hidden, int n_out, int ac_mode, int nonlin, const float *mean,
                                         const float *std, float *x, float *h1, float *h2, float *out, float *action) {
    if (n < 1 || !theta || !obs || !mean || !std || !x || !h1 || !h2 || !out || !action) { g_create_error = "dne_pendulum_forward_host: bad arguments"; return -1; }
    if (pendulum_shape_host("dne_pendulum_forward_host", hidden, n_out, ac_mode, nonlin)) return -1;
    pendulum::Options o{};
    fill_options(o, n_out, ac_mode, 0.0f, mean, std);
    const size_t P = pendulum::offsets(hidden, n_out).P;
    for (int i = 0; i < n; i++)
        action[i] = pendulum::forward_host(hidden, nonlin, theta + (size_t)i * P, o, obs + 3 * (size_t)i, x + 3 * (size_t)i, h1 + (size_t)i * hidden,
                                           h2 + (size_t)i * hidden, out + (size_t)i * n_out);
    return 0;
}

extern "C" int dne_pendulum_math_host(int fn, const double *x, int n, float a, float b, double *out) {
    if (fn < 0 || fn >= pendulum::MATH_FNS || n < 1 || !x || !out) { g_create_error = "dne_pendulum_math_host: bad arguments"; return -1; }
    for (int i = 0; i < n; i++) out[i] = pendulum::math_fn(fn, x[i], a, b);
    return 0;
}

// ------------------------------------------------------------------------------- MujocoPolicy on the hard maze (csrc/mjmaze.h)
extern "C" int dne_mjmaze_num_params(int hidden, int n_out) {
    if (!pendulum::hidden_ok(hidden) || n_out < mjmaze::ADIM || n_out > mjmaze::MAX_OUT || n_out % mjmaze::ADIM != 0) return -1;
    return mjmaze::offsets(hidden, n_out).P;
}

// what k_mjmaze_rollout reads for the members [first, first + count) of M (dne_set_members', or the GA bank's); the per-member options and the
// outputs are left null
static mjmaze::RolloutArgs mjmaze_args(dne_handle *h, const MazeMembers &M, int first, int count, int tslimit) {
    mjmaze::RolloutArgs A = member_args<mjmaze::RolloutArgs>(h, M, first, count, tslimit);
    A.hdr = h->maze_hdr; A.walls = h->maze_walls; A.nw = h->maze_nw; A.opt = h->mj_opt;
    return A;
}

static void mjmaze_launch(dne_handle *h, const mjmaze::RolloutArgs &A) {
    with_mujoco_shape(h, [&](auto H, auto TANH) { hipLaunchKernelGGL((mjmaze::k_mjmaze_rollout<H(), TANH()>), dim3(A.count), dim3(H()), 0, h->stream, A); });
}

extern "C" int dne_mjmaze_set_ob_stat(dne_handle *h, const float *mean, const float *std) {
    return mujoco_set_ob_stat(h, MJ_MAZE, "dne_mjmaze_set_ob_stat", mean, std);
}

extern "C" int dne_mjmaze_set_rollout_options(dne_handle *h, int n, float ac_noise_std, const int64_t *ac_off, const uint8_t *stat_flag) {
    return mujoco_set_rollout_options(h, MJ_MAZE, "dne_mjmaze_set_rollout_options", n, ac_noise_std, ac_off, stat_flag);
}

// what an evaluation and the trace ask alike before a launch
static int mjmaze_ready(dne_handle *h, const char *call) {
    if (h->maze_nw < 1) return h->fail("DNE_KIND_MJMAZE: no maze loaded (dne_maze_set_walls comes before an evaluation)");
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    return mujoco_stat_ready(h, MJ_MAZE, call);
}

// members [0, n) of M, one whole episode each from the header's start point (no reset seed: env_seed is not read), one launch
static int mjmaze_eval(dne_handle *h, const MazeMembers &M, const char *call, int n, int tslimit, float *returns, float *signreturns, int32_t *lengths, uint8_t *bc_out) {
    if (bc_out) return h->fail("%s: behaviour characterisations are not available on a DNE_KIND_MJMAZE engine (kind %d): bc must be NULL; "
                               "dne_maze_final_state has the final (x, y) of every member", call, DNE_KIND_MJMAZE);
    if (tslimit <= 0) return h->fail("timestep limit must be positive");
    if (mjmaze_ready(h, call) || mujoco_options_ready(h, MJ_MAZE, call, n)) return -1;
    mjmaze::RolloutArgs A = mjmaze_args(h, M, 0, n, tslimit);
    A.ret = h->ret; A.sign = h->sign; A.len = h->len; A.xy = h->maze_xy;
    mujoco_take_options(h, A);
    if (run_episodes(h, n, returns, signreturns, lengths, [&] { mjmaze_launch(h, A); })) return -1;
    h->maze_last_n = h->pd_last_n = n;
    return 0;
}

extern "C" int dne_mjmaze_ob_stats(dne_handle *h, int n, double *sum, double *sumsq, int32_t *count) {
    return mujoco_ob_stats(h, MJ_MAZE, "dne_mjmaze_ob_stats", n, sum, sumsq, count);
}

// the kernel once more for ONE of the current members, with every step written out: trace [min(tslimit, 400)][20] as dne_mjmaze_rollout_host
// writes it; no action noise, no statistics.  The accumulators of the last evaluation are left alone.
extern "C" int dne_mjmaze_debug_trace(dne_handle *h, int member, int tslimit, float *trace, int32_t *steps) {
    DeviceGuard dg(h);
    if (trace_args(h, "dne_mjmaze_debug_trace", DNE_KIND_MJMAZE, member, tslimit > 0 && trace && steps)) return -1;
    if (mjmaze_ready(h, "dne_mjmaze_debug_trace")) return -1;
    mjmaze::RolloutArgs A = mjmaze_args(h, maze_set_members(h), member, 1, tslimit);
    A.opt.ac_noise_std = 0.0f;
    return run_trace(h, "dne_mjmaze_debug_trace", std::min(tslimit, (int)mjmaze::EPISODE_STEPS), mjmaze::TRACE_W, trace, steps, [&](float *rows, int32_t *count) {
        A.trace = rows; A.trace_steps = count;
        mjmaze_launch(h, A);
    });
}

// the same header on the CPU: no handle, no GPU
static int mjmaze_shape_host(const char *call, int hidden, int n_out, int ac_mode, int nonlin) {
    return mujoco_shape_host(call, mjmaze::shape_ok(hidden, n_out, ac_mode, nonlin), hidden, n_out, ac_mode, nonlin, "mjmaze.h");
}

// one episode for each of n thetas [n][P] in the maze (header8, lines).  table / ac_off [n] (both or neither; an offset < 0: no noise for that
// member), stat_flag [n] or NULL: as the device call's options.  Outputs as the kernel writes them; trace [n][tslimit][20] or NULL.
extern "C" int dne_mjmaze_rollout_host(const float *theta, int n, int hidden, int n_out, int ac_mode, int nonlin, const float *mean, const float *std,
                                       const float *header8, const float *lines, int n_walls, int tslimit, float ac_noise_std, const float *table,
                                       size_t table_len, const int64_t *ac_off, const uint8_t *stat_flag, float *returns, float *signreturns,
                                       int32_t *lengths, float *xy, double *ob_sum, double *ob_sumsq, int32_t *ob_count, float *trace) {
    if (maze_check(&g_create_error, header8, lines, n_walls)) return -1;
    if (n < 1 || tslimit <= 0 || !theta || !mean || !std || !returns || !signreturns || !lengths || !xy || !ob_sum || !ob_sumsq || !ob_count ||
        (ac_off != nullptr) != (table != nullptr)) { g_create_error = "dne_mjmaze_rollout_host: bad arguments"; return -1; }
    if (mjmaze_shape_host("dne_mjmaze_rollout_host", hidden, n_out, ac_mode, nonlin)) return -1;
    mjmaze::Options o{};
    fill_options(o, n_out, ac_mode, ac_noise_std, mean, std);
    const size_t P = mjmaze::offsets(hidden, n_out).P;
    if (ac_off && ac_off_check_host("dne_mjmaze_rollout_host", ac_off, n, MJ_MAZE.ac_values, table_len)) return -1;
    const maze::Header m = maze_header(header8);
    for (int i = 0; i < n; i++) {
        const bool stat = stat_flag && stat_flag[i];
        const mjmaze::Episode e = mjmaze::rollout_host(hidden, nonlin, theta + (size_t)i * P, o, m, lines, n_walls, tslimit,
                                                       ac_off && ac_off[i] >= 0 ? table + ac_off[i] : nullptr, stat,
                                                       trace ? trace + (size_t)i * tslimit * mjmaze::TRACE_W : nullptr);
        returns[i] = e.ret; signreturns[i] = e.sign; lengths[i] = e.len;
        xy[2 * (size_t)i] = e.s.x; xy[2 * (size_t)i + 1] = e.s.y;
        for (int c = 0; c < mjmaze::OBS; c++) { ob_sum[mjmaze::OBS * (size_t)i + c] = e.ob_sum[c]; ob_sumsq[mjmaze::OBS * (size_t)i + c] = e.ob_sumsq[c]; }
        ob_count[i] = stat ? e.len : 0;
    }
    return 0;
}

// the policy alone: thetas [n][P] on raw observations [n][11] -> x [n][11] (normalised and clipped), h1 [n][H], h2 [n][H], out [n][n_out], action [n][2]
extern "C" int dne_mjmaze_forward_host(const float *theta, const float *obs, int n, int hidden, int n_out, int ac_mode, int nonlin, const float *mean,
                                       const float *std, float *x, float *h1, float *h2, float *out, float *action) {
    if (n < 1 || !theta || !obs || !mean || !std || !x || !h1 || !h2 || !out || !action) { g_create_error = "dne_mjmaze_forward_host: bad arguments"; return -1; }
    if (mjmaze_shape_host("dne_mjmaze_forward_host", hidden, n_out, ac_mode, nonlin)) return -1;
    mjmaze::Options o{};
    fill_options(o, n_out, ac_mode, 0.0f, mean, std);
    const size_t P = mjmaze::offsets(hidden, n_out).P;
    for (int i = 0; i < n; i++)
        mjmaze::forward_host(hidden, nonlin, theta + (size_t)i * P, o, obs + mjmaze::OBS * (size_t)i, x + mjmaze::OBS * (size_t)i, h1 + (size_t)i * hidden,
                             h2 + (size_t)i * hidden, out + (size_t)i * n_out, action + mjmaze::ADIM * (size_t)i);
    return 0;
}

// ------------------------------------------------------------------------------- Deep-GA on MujocoPolicy (csrc/mujoco_ga.h)
// maze_ga's bank for the two MujocoPolicy kinds: the halves hold T_max slots (dne_mujoco_ga_reserve), the roots of an evaluation get their
// scratch slots behind them when the first one comes, and a root's scale is one value a column, computed from its own noise slice
static int needs_mujoco(dne_handle *h, const char *call) {
    return (h->pendulum || h->mjmaze) ? 0 : h->fail("%s needs a DNE_KIND_PENDULUM or DNE_KIND_MJMAZE engine (this one: kind %d)", call, h->L.kind);
}

static float *mjg_bank(dne_handle *h, int half) { return h->mzg_mem + (size_t)half * h->mjg_Tmax * h->base_stride; }
static dim3 mjg_grid(dne_handle *h, int count) { return dim3(count, (h->mjg_L.P + 255) / 256); }

extern "C" int dne_mujoco_ga_reserve(dne_handle *h, int T_max) {
    DeviceGuard dg(h);
    if (needs_mujoco(h, "dne_mujoco_ga_reserve")) return -1;
    if (T_max < 1 || T_max > (1 << 20)) return h->fail("dne_mujoco_ga_reserve: T_max = %d outside [1, %d]", T_max, 1 << 20);
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, h->release(h->mzg_mem)); HCHECK(h, h->release(h->mzg_slot)); HCHECK(h, h->release(h->mzg_off)); HCHECK(h, h->release(h->mzg_scale));
    HCHECK(h, h->release(h->mjg_sc)); HCHECK(h, h->release(h->mjg_root_idx));
    // (the chain arrays too: chain_offs holds mjg_entries + 1 values, and mjg_entries follows T_max)
    HCHECK(h, h->release(h->mzg_chain_offs)); HCHECK(h, h->release(h->mzg_seeds)); HCHECK(h, h->release(h->mzg_powers));
    h->mzg_chain_cap = 0;
    h->mzg_T = h->mzg_half = h->mjg_Tmax = 0; h->mjg_root_cap = 0;
    h->mjg_L = mujoco_ga::layout(h->mjmaze ? (int)mjmaze::OBS : (int)pendulum::OBS, h->pd_hidden, h->cfg.n_actions);
    if (h->mjg_L.P != h->L.P) return h->fail("dne_mujoco_ga_reserve: the layout holds %d parameters, the engine %d", h->mjg_L.P, (int)h->L.P);
    h->mjg_sc_stride = (h->mjg_L.ncol + 15) / 16 * 16;
    h->mjg_entries = (size_t)std::max(h->M, T_max);
    const size_t E = h->mjg_entries, bank = 2 * (size_t)T_max * h->base_stride;
    HCHECK(h, h->alloc(&h->mzg_slot, E, "mujoco_ga_slot")); HCHECK(h, h->alloc(&h->mzg_off, E, "mujoco_ga_off")); HCHECK(h, h->alloc(&h->mzg_scale, E, "mujoco_ga_scale"));
    HCHECK(h, h->alloc(&h->mjg_sc, E * h->mjg_sc_stride, "mujoco_ga_colscale")); HCHECK(h, h->alloc(&h->mjg_root_idx, E, "mujoco_ga_root_idx"));
    float *mem = nullptr;
    HCHECK(h, h->alloc(&mem, bank, "mujoco_ga_bank"));
    HCHECK(h, hipMemset(mem, 0, bank * sizeof(float)));
    h->mzg_mem = mem; h->mjg_Tmax = T_max;
    return 0;
}

// what every call that reads the table or the bank needs first; an evaluation also its maze and its statistics
static int mjg_ready(dne_handle *h, const char *call, bool eval) {
    if (!h->mzg_mem) return h->fail("%s: no bank (dne_mujoco_ga_reserve comes first)", call);
    if (!h->noise) return h->fail("%s: noise table not uploaded (dne_noise_upload)", call);
    if (eval && h->mjmaze && h->maze_nw < 1) return h->fail("%s: no maze loaded (dne_maze_set_walls comes before an evaluation)", call);
    if (eval) return mujoco_stat_ready(h, h->mjmaze ? MJ_MAZE : MJ_PENDULUM, call);
    return 0;
}

// the column scales of entries [0, n): root[e] the noise index of entry e's root, < 0 for an entry without one
static int mjg_colscale(dne_handle *h, int n, const std::vector<int64_t> &root) {
    HCHECK(h, hipMemcpyAsync(h->mjg_root_idx, root.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(mujoco_ga::k_mujoco_ga_colscale, dim3(n, (h->mjg_L.ncol + 63) / 64), dim3(64), 0, h->stream, (const float *)h->noise, h->mjg_L,
                       (const int64_t *)h->mjg_root_idx, h->mjg_sc, h->mjg_sc_stride);
    HCHECK(h, hipGetLastError());
    return 0;
}

extern "C" int dne_mujoco_ga_build(dne_handle *h, int T, const int32_t *chain_offsets, const int64_t *seeds, const float *powers) {
    DeviceGuard dg(h);
    if (needs_mujoco(h, "dne_mujoco_ga_build")) return -1;
    if (mjg_ready(h, "dne_mujoco_ga_build", false)) return -1;
    if (T < 1 || T > h->mjg_Tmax) return h->fail("dne_mujoco_ga_build: T = %d outside [1, T_max = %d]", T, h->mjg_Tmax);
    if (!chain_offsets || !seeds || !powers) return h->fail("dne_mujoco_ga_build: a buffer is missing");
    if (chain_offsets[0] != 0) return h->fail("dne_mujoco_ga_build: chain_offsets starts at %d, not 0", chain_offsets[0]);
    const std::string bad = mujoco_ga::check_genomes(T, h->mjg_L.P, chain_offsets, seeds, h->noise_count);
    if (!bad.empty()) return h->fail("dne_mujoco_ga_build: %s", bad.c_str());
    const size_t total = (size_t)chain_offsets[T];
    if (total > h->mzg_chain_cap || !h->mzg_chain_offs) {
        HCHECK(h, hipStreamSynchronize(h->stream));
        HCHECK(h, h->release(h->mzg_chain_offs)); HCHECK(h, h->release(h->mzg_seeds)); HCHECK(h, h->release(h->mzg_powers));
        h->mzg_chain_cap = std::max<size_t>(2 * total, 4096);
        HCHECK(h, h->alloc(&h->mzg_chain_offs, h->mjg_entries + 1, "mujoco_ga_chain_offs"));
        HCHECK(h, h->alloc(&h->mzg_seeds, h->mzg_chain_cap, "mujoco_ga_seeds")); HCHECK(h, h->alloc(&h->mzg_powers, h->mzg_chain_cap, "mujoco_ga_powers"));
    }
    std::vector<int64_t> &root = h->mjg_host_root;
    root.resize(T);
    for (int j = 0; j < T; j++) root[j] = seeds[chain_offsets[j]];
    HCHECK(h, hipMemcpyAsync(h->mzg_chain_offs, chain_offsets, ((size_t)T + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->mzg_seeds, seeds, total * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->mzg_powers, powers, total * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (mjg_colscale(h, T, root)) return -1;
    const int other = 1 - h->mzg_half;
    hipLaunchKernelGGL(mujoco_ga::k_mujoco_ga_build, mjg_grid(h, T), dim3(256), 0, h->stream, (const float *)h->noise, h->mjg_L, (const float *)h->mjg_sc,
                       h->mjg_sc_stride, (const int32_t *)h->mzg_chain_offs, (const int64_t *)h->mzg_seeds, (const float *)h->mzg_powers, mjg_bank(h, other),
                       h->base_stride);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));   // the caller's arrays may go away
    h->mzg_half = other; h->mzg_T = T;
    return 0;
}

extern "C" int dne_mujoco_ga_promote(dne_handle *h, int T_new, const int32_t *parent, const int64_t *idx, const float *power) {
    DeviceGuard dg(h);
    if (needs_mujoco(h, "dne_mujoco_ga_promote")) return -1;
    if (mjg_ready(h, "dne_mujoco_ga_promote", false)) return -1;
    if (T_new < 1 || T_new > h->mjg_Tmax) return h->fail("dne_mujoco_ga_promote: T = %d outside [1, T_max = %d]", T_new, h->mjg_Tmax);
    if (!parent || !idx || !power) return h->fail("dne_mujoco_ga_promote: a buffer is missing");
    std::vector<int64_t> &root = h->mjg_host_root;
    root.resize(T_new);
    bool roots = false;
    for (int j = 0; j < T_new; j++) {
        const std::string bad = mujoco_ga::check_member(j, h->mzg_T, h->mjg_L.P, h->noise_count, parent[j], idx[j], true);
        if (!bad.empty()) return h->fail("dne_mujoco_ga_promote: %s", bad.c_str());
        root[j] = parent[j] < 0 ? idx[j] : -1;
        roots = roots || parent[j] < 0;
    }
    if (mzg_upload_members(h, T_new, parent, idx, power)) return -1;
    if (roots && mjg_colscale(h, T_new, root)) return -1;
    const int other = 1 - h->mzg_half;
    hipLaunchKernelGGL(mujoco_ga::k_mujoco_ga_promote, mjg_grid(h, T_new), dim3(256), 0, h->stream, (const float *)h->noise, h->mjg_L, (const float *)h->mjg_sc,
                       h->mjg_sc_stride, (const float *)mjg_bank(h, h->mzg_half), mjg_bank(h, other), h->base_stride, (const int32_t *)h->mzg_slot,
                       (const int64_t *)h->mzg_off, (const float *)h->mzg_scale);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->mzg_half = other; h->mzg_T = T_new;
    return 0;
}

// the scratch slots of an evaluation's roots, behind the two halves of the bank: `need` of them, the bank carried over when they grow
static int mjg_root_slots(dne_handle *h, size_t need) {
    if (need <= h->mjg_root_cap) return 0;
    const size_t bank = 2 * (size_t)h->mjg_Tmax * h->base_stride, all = bank + need * h->base_stride;
    float *mem = nullptr;
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, h->alloc(&mem, all, "mujoco_ga_bank"));
    HCHECK(h, hipMemcpy(mem, h->mzg_mem, bank * sizeof(float), hipMemcpyDeviceToDevice));
    HCHECK(h, hipMemset(mem + bank, 0, (all - bank) * sizeof(float)));
    HCHECK(h, h->release(h->mzg_mem));
    h->mzg_mem = mem; h->mjg_root_cap = need;
    return 0;
}

extern "C" int dne_mujoco_ga_eval(dne_handle *h, int n, const int32_t *parent, const int64_t *idx, const float *power, const uint32_t *env_seed, int tslimit,
                                  float *returns, float *signreturns, int32_t *lengths) {
    DeviceGuard dg(h);
    if (needs_mujoco(h, "dne_mujoco_ga_eval")) return -1;
    if (mjg_ready(h, "dne_mujoco_ga_eval", true)) return -1;
    if (n < 1 || n > h->M) return h->fail("dne_mujoco_ga_eval: n = %d outside [1, max_members = %d]", n, h->M);
    if (!parent || !idx || !power || !returns || !lengths) return h->fail("dne_mujoco_ga_eval: a buffer is missing");
    if (tslimit <= 0) return h->fail("dne_mujoco_ga_eval: timestep limit must be positive");
    if (h->pendulum && !env_seed) return h->fail("dne_mujoco_ga_eval: a DNE_KIND_PENDULUM engine resets every member from its environment seed, env_seed is NULL");
    // a child is the rollout kernel's own member: (its parent's bank slot, idx, power); a root runs from scratch slot 2 T_max + i at scale 0
    const int bank0 = h->mzg_half * h->mjg_Tmax, root0 = 2 * h->mjg_Tmax;
    std::vector<int32_t> &slot = h->mzg_host_slot;
    std::vector<float> &scale = h->mzg_host_scale;
    std::vector<int64_t> &rootidx = h->mjg_host_root;
    slot.resize(n); scale.resize(n); rootidx.resize(n);
    bool roots = false;
    for (int i = 0; i < n; i++) {
        const std::string bad = mujoco_ga::check_member(i, h->mzg_T, h->mjg_L.P, h->noise_count, parent[i], idx[i], false);
        if (!bad.empty()) return h->fail("dne_mujoco_ga_eval: %s", bad.c_str());
        const bool root = parent[i] < 0;
        slot[i] = root ? root0 + i : bank0 + parent[i];
        scale[i] = root ? 0.0f : power[i];
        rootidx[i] = root ? idx[i] : -1;
        roots = roots || root;
    }
    if (mujoco_options_ready(h, h->mjmaze ? MJ_MAZE : MJ_PENDULUM, "dne_mujoco_ga_eval", n)) return -1;
    if (roots && mjg_root_slots(h, (size_t)n)) return -1;
    if (mzg_upload_members(h, n, slot.data(), idx, scale.data())) return -1;
    if (roots) {
        if (mjg_colscale(h, n, rootidx)) return -1;
        hipLaunchKernelGGL(mujoco_ga::k_mujoco_ga_roots, mjg_grid(h, n), dim3(256), 0, h->stream, (const float *)h->noise, h->mjg_L, (const float *)h->mjg_sc,
                           h->mjg_sc_stride, (const int32_t *)h->mzg_slot, (const int64_t *)h->mzg_off, root0, h->mzg_mem, h->base_stride);
        HCHECK(h, hipGetLastError());
    }
    const MazeMembers M{h->mzg_mem, h->mzg_slot, h->mzg_off, h->mzg_scale};
    if (h->pendulum) return pendulum_eval(h, M, "dne_mujoco_ga_eval", n, tslimit, env_seed, returns, signreturns, lengths, nullptr);
    return mjmaze_eval(h, M, "dne_mujoco_ga_eval", n, tslimit, returns, signreturns, lengths, nullptr);
}

extern "C" int dne_mujoco_ga_parents(dne_handle *h) {
    if (needs_mujoco(h, "dne_mujoco_ga_parents")) return -1;
    return h->mzg_T;
}

extern "C" int dne_mujoco_ga_get_parent(dne_handle *h, int j, float *out) {
    DeviceGuard dg(h);
    if (needs_mujoco(h, "dne_mujoco_ga_get_parent")) return -1;
    if (!h->mzg_mem) return h->fail("dne_mujoco_ga_get_parent: no bank (dne_mujoco_ga_reserve comes first)");
    if (j < 0 || j >= h->mzg_T) return h->fail("dne_mujoco_ga_get_parent: parent %d, the bank holds %d", j, h->mzg_T);
    if (!out) return h->fail("dne_mujoco_ga_get_parent: no output buffer");
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, mjg_bank(h, h->mzg_half) + (size_t)j * h->base_stride, (size_t)h->mjg_L.P * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// the same header on the CPU: no handle, no GPU
static int mjg_host_layout(const char *call, int kind, int hidden, int n_out, const float *noise, size_t count, mujoco_ga::Layout *L) {
    const std::string c(call);
    if (kind != DNE_KIND_PENDULUM && kind != DNE_KIND_MJMAZE) {
        g_create_error = c + ": kind " + std::to_string(kind) + " runs no MujocoPolicy (DNE_KIND_PENDULUM (6) and DNE_KIND_MJMAZE (7) do)";
        return -1;
    }
    const int obs = kind == DNE_KIND_MJMAZE ? (int)mjmaze::OBS : (int)pendulum::OBS;
    if (!mujoco_ga::shape_ok(obs, hidden, n_out)) {
        g_create_error = c + ": hidden width " + std::to_string(hidden) + " with " + std::to_string(n_out) + " outputs is not a shape csrc/" +
                         (kind == DNE_KIND_MJMAZE ? "mjmaze.h" : "pendulum.h") + " builds";
        return -1;
    }
    *L = mujoco_ga::layout(obs, hidden, n_out);
    if (!noise) { g_create_error = c + ": a buffer is missing"; return -1; }
    if (count < (size_t)L->P) { g_create_error = c + ": a table of " + std::to_string(count) + " floats holds no P = " + std::to_string(L->P) + " parameters"; return -1; }
    return 0;
}

extern "C" int dne_mujoco_ga_colscale_host(const float *noise, size_t count, int kind, int hidden, int n_out, int64_t idx0, float *out) {
    mujoco_ga::Layout L;
    if (mjg_host_layout("dne_mujoco_ga_colscale_host", kind, hidden, n_out, noise, count, &L)) return -1;
    if (!out) { g_create_error = "dne_mujoco_ga_colscale_host: a buffer is missing"; return -1; }
    if (!dense_ga::in_table(idx0, L.P, count)) {
        g_create_error = "dne_mujoco_ga_colscale_host: " + dense_ga::fmt("noise index %lld + P = %lld outside the table of %lld", (long long)idx0, L.P, (long long)count);
        return -1;
    }
    mujoco_ga::colscale_host(noise, L, idx0, out);
    return 0;
}

extern "C" int dne_mujoco_ga_theta_host(const float *noise, size_t count, int kind, int hidden, int n_out, const int64_t *seeds, const float *powers, int nseeds,
                                        float *out) {
    mujoco_ga::Layout L;
    if (mjg_host_layout("dne_mujoco_ga_theta_host", kind, hidden, n_out, noise, count, &L)) return -1;
    if (!seeds || !powers || !out) { g_create_error = "dne_mujoco_ga_theta_host: a buffer is missing"; return -1; }
    const int32_t co[2] = {0, nseeds};
    const std::string bad = mujoco_ga::check_genomes(1, L.P, co, seeds, count);
    if (!bad.empty()) { g_create_error = "dne_mujoco_ga_theta_host: " + bad; return -1; }
    mujoco_ga::genome_host(noise, L, seeds, powers, nseeds, out);
    return 0;
}

extern "C" int dne_mujoco_ga_members_host(const float *noise, size_t count, int kind, int hidden, int n_out, const float *bank, int T, const int32_t *parent,
                                          const int64_t *idx, const float *power, int n, float *out) {
    mujoco_ga::Layout L;
    if (mjg_host_layout("dne_mujoco_ga_members_host", kind, hidden, n_out, noise, count, &L)) return -1;
    if (n < 1) { g_create_error = "dne_mujoco_ga_members_host: n = " + std::to_string(n) + ", at least one member is needed"; return -1; }
    if (T < 0 || (T > 0 && !bank)) { g_create_error = "dne_mujoco_ga_members_host: T = " + std::to_string(T) + " parents without a bank"; return -1; }
    if (!parent || !idx || !power || !out) { g_create_error = "dne_mujoco_ga_members_host: a buffer is missing"; return -1; }
    for (int i = 0; i < n; i++) {
        const std::string bad = mujoco_ga::check_member(i, T, L.P, count, parent[i], idx[i], true);
        if (!bad.empty()) { g_create_error = "dne_mujoco_ga_members_host: " + bad; return -1; }
    }
    mujoco_ga::members_host(noise, L, bank, parent, idx, power, n, out);
    return 0;
}

// ------------------------------------------------------------------------------- environments stepped by the caller (csrc/step_env.h)
static_assert(stepenv::KIND_MAZE == DNE_KIND_MAZE && stepenv::KIND_CARTPOLE == DNE_KIND_CARTPOLE && stepenv::KIND_PENDULUM == DNE_KIND_PENDULUM,
              "step_env.h restates the three kinds");
static_assert(stepenv::ENV_ACROBOT == DNE_ENV_ACROBOT, "step_env.h restates the environment id");

extern "C" int dne_stepenv_dims(int kind, int *obs, int *act, int *state, int *act_is_int) {
    stepenv::Dims d;
    if (!stepenv::dims(kind, &d)) {
        g_create_error = "dne_stepenv_dims: kind " + std::to_string(kind) + " has no step-at-a-time environment (DNE_KIND_MAZE, DNE_KIND_CARTPOLE and DNE_KIND_PENDULUM have, and the id DNE_ENV_ACROBOT)";
        return -1;
    }
    if (obs) *obs = d.obs;
    if (act) *act = d.act;
    if (state) *state = d.state;
    if (act_is_int) *act_is_int = d.act_is_int;
    return 0;
}

// the environment a handle steps: its kind, or what a DNE_KIND_DENSE engine was created on
static int se_env(const dne_handle *h) { return h->dense ? h->dn_shape.env : h->L.kind; }
static stepenv::Dims se_dims(const dne_handle *h) {
    stepenv::Dims d{};
    stepenv::dims(se_env(h), &d);
    return d;
}

static stepenv::MazeCtx se_maze_ctx(const dne_handle *h) { return {h->maze_hdr, h->maze_walls, h->maze_nw}; }

// the batch, at the first call that needs it: every environment starts as zeros and "never reset"
static int se_alloc(dne_handle *h) {
    if (h->se_ready) return 0;
    const size_t M = h->M;
    const stepenv::Dims d = se_dims(h);
    HCHECK(h, h->alloc(&h->se.state, M * d.state, "stepenv_state")); HCHECK(h, h->alloc(&h->se.steps, M, "stepenv_steps"));
    HCHECK(h, h->alloc(&h->se.limit, M, "stepenv_limit")); HCHECK(h, h->alloc(&h->se.done, M, "stepenv_done"));
    HCHECK(h, h->alloc(&h->se.obs, M * d.obs, "stepenv_obs"));
    HCHECK(h, hipMemset(h->se.state, 0, M * d.state * sizeof(double))); HCHECK(h, hipMemset(h->se.steps, 0, M * sizeof(int32_t)));
    HCHECK(h, hipMemset(h->se.limit, 0, M * sizeof(int32_t))); HCHECK(h, hipMemset(h->se.done, 0, M)); HCHECK(h, hipMemset(h->se.obs, 0, M * d.obs * sizeof(float)));
    HCHECK(h, h->alloc(&h->se_io_idx, M, "stepenv_io_idx")); HCHECK(h, h->alloc(&h->se_io_steps, M, "stepenv_io_steps"));
    HCHECK(h, h->alloc(&h->se_io_seeds, M, "stepenv_io_seeds")); HCHECK(h, h->alloc(&h->se_io_act, M * stepenv::MAX_ACT, "stepenv_io_act"));
    HCHECK(h, h->alloc(&h->se_io_rew, M, "stepenv_io_rew")); HCHECK(h, h->alloc(&h->se_io_obs, M * d.obs, "stepenv_io_obs"));
    HCHECK(h, h->alloc(&h->se_io_done, M, "stepenv_io_done")); HCHECK(h, h->alloc(&h->se_io_state, M * d.state, "stepenv_io_state"));
    if (h->dense) { HCHECK(h, h->alloc(&h->se_io_mem, M, "stepenv_io_mem")); HCHECK(h, h->alloc(&h->se_io_out, M * dense::MAX_OUT, "stepenv_io_out")); }
    HCHECK(h, hipEventCreate(&h->se_ev_a)); HCHECK(h, hipEventCreate(&h->se_ev_b));
    h->se_was_reset.assign(M, 0);
    h->se_ready = true;
    return 0;
}

// What every dne_stepenv_* call on a handle asks first: the kind, the maze's walls, n, the index list (NULL = 0 .. n - 1) in range and without
// a repeat, and -- for a call that reads environments -- that each was reset.  Fills idx.  A refusal comes before anything on the device moves.
static int se_check(dne_handle *h, const char *call, int n, const int32_t *indices, bool reads, std::vector<int32_t> &idx) {
    if (!h->episodic() || h->mjmaze)   // (DNE_KIND_MJMAZE: the maze one step at a time is DNE_KIND_MAZE's)
        return h->fail("%s needs a DNE_KIND_MAZE, DNE_KIND_CARTPOLE or DNE_KIND_PENDULUM engine (this one: kind %d)", call, h->L.kind);
    if (se_env(h) == DNE_KIND_MAZE && h->maze_nw < 1) return h->fail("%s: no maze loaded (dne_maze_set_walls comes before the environments)", call);
    if (n < 1 || n > h->M) return h->fail("%s: %d environments asked for, the engine holds 1..%d", call, n, h->M);
    idx.resize(n);
    std::vector<uint8_t> seen(h->M, 0);
    for (int i = 0; i < n; i++) {
        const int e = indices ? indices[i] : i;
        if (e < 0 || e >= h->M) return h->fail("%s: index %d at position %d is out of range, the engine holds environments 0..%d", call, e, i, h->M - 1);
        if (seen[e]) return h->fail("%s: environment %d is named twice", call, e);
        seen[e] = 1;
        idx[i] = e;
    }
    if (reads)
        for (int i = 0; i < n; i++)
            if (!h->se_ready || !h->se_was_reset[idx[i]])
                return h->fail("%s: environment %d was never reset (dne_stepenv_reset or dne_stepenv_set_state comes first)", call, idx[i]);
    return 0;
}

// dne_stepenv_reset (state == NULL) and dne_stepenv_set_state: one launch of the kind's reset kernel over the list
static int se_reset(dne_handle *h, const char *call, int n, const int32_t *indices, const uint32_t *seeds, const double *state, const int32_t *steps,
                    int max_steps, bool set) {
    std::vector<int32_t> idx;
    if (se_check(h, call, n, indices, false, idx)) return -1;
    const stepenv::Dims d = se_dims(h);
    const bool is_maze = se_env(h) == DNE_KIND_MAZE, is_cartpole = se_env(h) == DNE_KIND_CARTPOLE, is_acrobot = se_env(h) == DNE_ENV_ACROBOT;
    const int limit = stepenv::step_limit(max_steps, d.own_limit);
    if (set) {
        if (!state || !steps) return h->fail("%s: state or steps missing", call);
        for (int i = 0; i < n; i++)
            if (steps[i] < 0 || steps[i] >= limit)
                return h->fail("%s: %d steps taken at position %d, an environment under a limit of %d has taken 0..%d", call, steps[i], i, limit, limit - 1);
    } else if (!is_maze && !seeds)
        return h->fail("%s: a %s engine resets every environment from its seed, seeds is NULL", call, episodic_kind_name(se_env(h)));
    if (se_alloc(h)) return -1;
    HCHECK(h, hipMemcpyAsync(h->se_io_idx, idx.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (set) {
        HCHECK(h, hipMemcpyAsync(h->se_io_state, state, (size_t)n * d.state * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HCHECK(h, hipMemcpyAsync(h->se_io_steps, steps, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    } else if (!is_maze)
        HCHECK(h, hipMemcpyAsync(h->se_io_seeds, seeds, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    const double *init = set ? h->se_io_state : nullptr;
    if (is_maze)
        hipLaunchKernelGGL(stepenv::k_stepenv_reset_maze, dim3((n + 3) / 4), dim3(64), 0, h->stream, h->se, se_maze_ctx(h), h->se_io_idx, n, init, h->se_io_steps, limit);
    else if (is_cartpole)
        hipLaunchKernelGGL(stepenv::k_stepenv_reset_cartpole, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->se, h->se_io_idx, n, h->se_io_seeds, init, h->se_io_steps, limit);
    else if (is_acrobot)
        hipLaunchKernelGGL(stepenv::k_stepenv_reset_acrobot, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->se, h->se_io_idx, n, h->se_io_seeds, init, h->se_io_steps, limit);
    else
        hipLaunchKernelGGL(stepenv::k_stepenv_reset_pendulum, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->se, h->se_io_idx, n, h->se_io_seeds, init, h->se_io_steps, limit);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++) h->se_was_reset[idx[i]] = 1;
    return 0;
}

extern "C" int dne_stepenv_reset(dne_handle *h, int n, const int32_t *indices, const uint32_t *seeds, int max_steps) {
    DeviceGuard dg(h);
    return se_reset(h, "dne_stepenv_reset", n, indices, seeds, nullptr, nullptr, max_steps, false);
}

extern "C" int dne_stepenv_set_state(dne_handle *h, int n, const int32_t *indices, const double *state, const int32_t *steps, int max_steps) {
    DeviceGuard dg(h);
    return se_reset(h, "dne_stepenv_set_state", n, indices, nullptr, state, steps, max_steps, true);
}

static int se_step(dne_handle *h, const char *call, bool int_actions, int n, const int32_t *indices, const void *actions, float *reward, uint8_t *done) {
    std::vector<int32_t> idx;
    if (se_check(h, call, n, indices, true, idx)) return -1;
    const stepenv::Dims d = se_dims(h);
    const bool is_maze = se_env(h) == DNE_KIND_MAZE, is_cartpole = se_env(h) == DNE_KIND_CARTPOLE, is_acrobot = se_env(h) == DNE_ENV_ACROBOT;
    if ((d.act_is_int != 0) != int_actions)
        return h->fail("%s: a %s engine takes %s actions (dne_stepenv_step_%s)", call, episodic_kind_name(se_env(h)), d.act_is_int ? "int32" : "float",
                       d.act_is_int ? "i32" : "f32");
    if (!actions || !reward || !done) return h->fail("%s: actions, reward or done missing", call);
    if (is_cartpole)
        for (int i = 0; i < n; i++) {
            const int32_t a = ((const int32_t *)actions)[i];
            if (a != 0 && a != 1) return h->fail("%s: action %d at position %d, CartPole-v1 has actions 0 and 1", call, a, i);
        }
    if (is_acrobot)
        for (int i = 0; i < n; i++) {
            const int32_t a = ((const int32_t *)actions)[i];
            if (a < 0 || a > 2) return h->fail("%s: action %d at position %d, Acrobot-v1 has actions 0, 1 and 2", call, a, i);
        }
    HCHECK(h, hipMemcpyAsync(h->se_io_idx, idx.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->se_io_act, actions, (size_t)n * d.act * sizeof(float), hipMemcpyHostToDevice, h->stream));   // (an int32 is a float's size)
    HCHECK(h, hipEventRecord(h->se_ev_a, h->stream));
    if (is_maze)
        hipLaunchKernelGGL(stepenv::k_stepenv_step_maze, dim3((n + 3) / 4), dim3(64), 0, h->stream, h->se, se_maze_ctx(h), h->se_io_idx, n, h->se_io_act, h->se_io_rew, h->se_io_done);
    else if (is_cartpole)
        hipLaunchKernelGGL(stepenv::k_stepenv_step_cartpole, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->se, h->se_io_idx, n, (const int32_t *)h->se_io_act, h->se_io_rew, h->se_io_done);
    else if (is_acrobot)
        hipLaunchKernelGGL(stepenv::k_stepenv_step_acrobot, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->se, h->se_io_idx, n, (const int32_t *)h->se_io_act, h->se_io_rew, h->se_io_done);
    else
        hipLaunchKernelGGL(stepenv::k_stepenv_step_pendulum, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->se, h->se_io_idx, n, h->se_io_act, h->se_io_rew, h->se_io_done);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->se_ev_b, h->stream));
    HCHECK(h, hipMemcpyAsync(reward, h->se_io_rew, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipMemcpyAsync(done, h->se_io_done, n, hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->se_ev_a, h->se_ev_b));
    h->se_last_ms = ms;
    return 0;
}

extern "C" int dne_stepenv_step_f32(dne_handle *h, int n, const int32_t *indices, const float *actions, float *reward, uint8_t *done) {
    DeviceGuard dg(h);
    return se_step(h, "dne_stepenv_step_f32", false, n, indices, actions, reward, done);
}

extern "C" int dne_stepenv_step_i32(dne_handle *h, int n, const int32_t *indices, const int32_t *actions, float *reward, uint8_t *done) {
    DeviceGuard dg(h);
    return se_step(h, "dne_stepenv_step_i32", true, n, indices, actions, reward, done);
}

// k_stepenv_gather over the list: whichever of the outputs is not NULL
static int se_gather(dne_handle *h, const char *call, int n, const int32_t *indices, float *obs, double *state, int32_t *steps, uint8_t *done) {
    std::vector<int32_t> idx;
    if (se_check(h, call, n, indices, true, idx)) return -1;
    const stepenv::Dims d = se_dims(h);
    HCHECK(h, hipMemcpyAsync(h->se_io_idx, idx.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(stepenv::k_stepenv_gather, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->se, d.state, d.obs, h->se_io_idx, n, obs ? h->se_io_obs : nullptr,
                       state ? h->se_io_state : nullptr, steps ? h->se_io_steps : nullptr, done ? h->se_io_done : nullptr);
    HCHECK(h, hipGetLastError());
    if (obs) HCHECK(h, hipMemcpyAsync(obs, h->se_io_obs, (size_t)n * d.obs * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (state) HCHECK(h, hipMemcpyAsync(state, h->se_io_state, (size_t)n * d.state * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (steps) HCHECK(h, hipMemcpyAsync(steps, h->se_io_steps, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (done) HCHECK(h, hipMemcpyAsync(done, h->se_io_done, n, hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int dne_stepenv_observation(dne_handle *h, int n, const int32_t *indices, float *obs) {
    DeviceGuard dg(h);
    if (!obs) return h->fail("dne_stepenv_observation: no output buffer");
    return se_gather(h, "dne_stepenv_observation", n, indices, obs, nullptr, nullptr, nullptr);
}

extern "C" int dne_stepenv_get_state(dne_handle *h, int n, const int32_t *indices, double *state, int32_t *steps, uint8_t *done) {
    DeviceGuard dg(h);
    if (!state && !steps && !done) return h->fail("dne_stepenv_get_state: no output buffer");
    return se_gather(h, "dne_stepenv_get_state", n, indices, nullptr, state, steps, done);
}

extern "C" double dne_stepenv_last_ms(dne_handle *h) { return h->episodic() ? h->se_last_ms : -1.0; }

// the same header on the CPU: no handle, no GPU
static int se_host_args(const char *call, int kind, int n, const float *header8, const float *lines, int n_walls, stepenv::MazeCtx *mz) {
    stepenv::Dims d;
    if (!stepenv::dims(kind, &d)) {
        g_create_error = std::string(call) + ": kind " + std::to_string(kind) + " has no step-at-a-time environment (DNE_KIND_MAZE, DNE_KIND_CARTPOLE and DNE_KIND_PENDULUM have, and the id DNE_ENV_ACROBOT)";
        return -1;
    }
    if (n < 1) { g_create_error = std::string(call) + ": n = " + std::to_string(n) + ", at least one environment is needed"; return -1; }
    if (kind == DNE_KIND_MAZE) {
        if (maze_check(&g_create_error, header8, lines, n_walls)) { g_create_error = std::string(call) + ": " + g_create_error; return -1; }
        mz->hdr = maze_header(header8); mz->walls = lines; mz->nw = n_walls;
    }
    return 0;
}

extern "C" int dne_stepenv_reset_host(int kind, int n, const uint32_t *seeds, const float *header8, const float *lines, int n_walls, int max_steps,
                                      double *state, int32_t *steps, int32_t *limit, uint8_t *done, float *obs) {
    stepenv::MazeCtx mz{};
    if (se_host_args("dne_stepenv_reset_host", kind, n, header8, lines, n_walls, &mz)) return -1;
    if (!state || !steps || !limit || !done || !obs) { g_create_error = "dne_stepenv_reset_host: an output buffer is missing"; return -1; }
    if (kind != DNE_KIND_MAZE && !seeds) { g_create_error = std::string("dne_stepenv_reset_host: ") + episodic_kind_name(kind) + " resets every environment from its seed, seeds is NULL"; return -1; }
    return stepenv::reset_host(kind, n, seeds, &mz, max_steps, state, steps, limit, done, obs);
}

extern "C" int dne_stepenv_step_host(int kind, int n, const void *actions, const float *header8, const float *lines, int n_walls, double *state,
                                     int32_t *steps, const int32_t *limit, uint8_t *done, float *reward, float *obs) {
    stepenv::MazeCtx mz{};
    if (se_host_args("dne_stepenv_step_host", kind, n, header8, lines, n_walls, &mz)) return -1;
    if (!actions || !state || !steps || !limit || !done || !reward || !obs) { g_create_error = "dne_stepenv_step_host: a buffer is missing"; return -1; }
    if (stepenv::step_host(kind, n, actions, &mz, state, steps, limit, done, reward, obs) == -2) {
        for (int i = 0; i < n; i++) {
            const int32_t a = ((const int32_t *)actions)[i];
            if (kind == DNE_ENV_ACROBOT) {
                if (a < 0 || a > 2) { g_create_error = "dne_stepenv_step_host: action " + std::to_string(a) + " at position " + std::to_string(i) + ", Acrobot-v1 has actions 0, 1 and 2"; break; }
            } else if (a != 0 && a != 1) { g_create_error = "dne_stepenv_step_host: action " + std::to_string(a) + " at position " + std::to_string(i) + ", CartPole-v1 has actions 0 and 1"; break; }
        }
        return -1;
    }
    return 0;
}

extern "C" int dne_acrobot_actions_host(const int32_t *actions, int n, int T, const double *init4, double *rows) {
    if (n < 1 || T < 1 || !actions || !init4 || !rows) { g_create_error = "dne_acrobot_actions_host: bad arguments"; return -1; }
    for (size_t i = 0; i < (size_t)n * T; i++)
        if (actions[i] < 0 || actions[i] > 2) { g_create_error = "dne_acrobot_actions_host: action " + std::to_string(actions[i]) + ", Acrobot-v1 has actions 0, 1 and 2"; return -1; }
    for (int i = 0; i < n; i++) acrobot::actions_host(actions + (size_t)i * T, T, init4 + 4 * (size_t)i, rows + (size_t)i * T * 5);
    return 0;
}

extern "C" int dne_stepenv_observe_host(int kind, int n, const double *state, const float *header8, const float *lines, int n_walls, float *obs) {
    stepenv::MazeCtx mz{};
    if (se_host_args("dne_stepenv_observe_host", kind, n, header8, lines, n_walls, &mz)) return -1;
    if (!state || !obs) { g_create_error = "dne_stepenv_observe_host: a buffer is missing"; return -1; }
    return stepenv::observe_host(kind, n, state, &mz, obs);
}


// ------------------------------------------------------------------------------- dense policies on the step environments (csrc/dense.h)
static void dense_launch(dne_handle *h, int items, const dense::RunArgs &A) {
    const size_t lds = (size_t)A.shape.P * sizeof(float);
    if (A.shape.env == DNE_KIND_MAZE) hipLaunchKernelGGL(dense::k_dense_run<DNE_KIND_MAZE>, dim3(items), dim3(64), lds, h->stream, A);
    else if (A.shape.env == DNE_KIND_CARTPOLE) hipLaunchKernelGGL(dense::k_dense_run<DNE_KIND_CARTPOLE>, dim3(items), dim3(64), lds, h->stream, A);
    else if (A.shape.env == DNE_KIND_PENDULUM) hipLaunchKernelGGL(dense::k_dense_run<DNE_KIND_PENDULUM>, dim3(items), dim3(64), lds, h->stream, A);
    else hipLaunchKernelGGL(dense::k_dense_run<DNE_ENV_ACROBOT>, dim3(items), dim3(64), lds, h->stream, A);
}

// what k_dense_run reads whatever it is used for: the members M (dne_set_members', or the GA bank's), the shape, the maze
static dense::RunArgs dense_args(dne_handle *h, const MazeMembers &M) {
    dense::RunArgs A{};
    A.noise = h->noise; A.bases = M.bases; A.base_stride = h->base_stride;
    A.m_slot = M.slot; A.m_off = M.off; A.m_scale = M.scale;
    A.shape = h->dn_shape;
    A.C = se_maze_ctx(h);
    return A;
}

static const char *dense_env_name(int env) { return env == DNE_KIND_CARTPOLE ? "cart-pole" : env == DNE_ENV_ACROBOT ? "acrobot" : "pendulum"; }

// members [0, n) of M, one whole episode each from its own reset, one launch; the step-at-a-time batch is not touched
static int dense_eval(dne_handle *h, const MazeMembers &M, const char *call, int n, int tslimit, const uint32_t *env_seed, float *returns, float *signreturns,
                      int32_t *lengths, uint8_t *bc_out) {
    const bool is_maze = h->dn_shape.env == DNE_KIND_MAZE;
    if (bc_out) return h->fail("%s: behaviour characterisations are not available on a DNE_KIND_DENSE engine (kind %d): bc must be NULL; "
                               "dne_dense_final_state has the final state of every member", call, DNE_KIND_DENSE);
    if (tslimit <= 0) return h->fail("timestep limit must be positive");
    if (is_maze && h->maze_nw < 1) return h->fail("DNE_KIND_DENSE: no maze loaded (dne_maze_set_walls comes before an evaluation)");
    if (!is_maze && !env_seed) return h->fail("%s: a DNE_KIND_DENSE engine on the %s resets every member from its environment seed, env_seed is NULL", call,
                                              dense_env_name(h->dn_shape.env));
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    if (!is_maze) HCHECK(h, hipMemcpyAsync(h->seeds, env_seed, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    dense::RunArgs A = dense_args(h, M);
    A.seed = h->seeds; A.episode = 1; A.max_steps = tslimit;
    A.ret = h->ret; A.sign = h->sign; A.steps_out = h->len; A.state_out = h->dn_state;
    h->dn_bc_valid = false;   // (whatever the launch leaves in dn_state, the BCs formed from the evaluation before are not its)
    if (run_episodes(h, n, returns, signreturns, lengths, [&] { dense_launch(h, n, A); })) return -1;
    h->dn_last_n = n;
    return 0;
}

extern "C" int dne_dense_env_kind(dne_handle *h) { return se_env(h); }

extern "C" int dne_dense_final_state(dne_handle *h, int n, double *state) {
    DeviceGuard dg(h);
    if (!h->dense) return h->fail("dne_dense_final_state needs a DNE_KIND_DENSE engine (this one: kind %d)", h->L.kind);
    return last_eval_rows(h, "dne_dense_final_state", n, h->dn_last_n, state != nullptr, state, (const double *)h->dn_state, se_dims(h).state);
}

// dne_stepenv_act (max_steps == 0) and dne_stepenv_run: the policy of members[i] behind environment indices[i], one k_dense_run launch
static int se_dense(dne_handle *h, const char *call, bool run, int n, const int32_t *indices, const int32_t *members, int max_steps, float *out, void *actions,
                    float *reward_sum, int32_t *steps_taken, uint8_t *done) {
    if (!h->dense) return h->fail("%s needs a DNE_KIND_DENSE engine (this one: kind %d)", call, h->L.kind);
    if (run && max_steps < 1) return h->fail("%s: max_steps = %d, at least one act -> step round is needed", call, max_steps);
    std::vector<int32_t> idx;
    if (se_check(h, call, n, indices, true, idx)) return -1;
    const int set = (int)h->host_slot.size();
    if (set < 1) return h->fail("%s: no members set (dne_set_members comes before the policy)", call);
    std::vector<int32_t> mem(n);
    for (int i = 0; i < n; i++) {
        mem[i] = members ? members[i] : idx[i];
        if (mem[i] < 0 || mem[i] >= set) return h->fail("%s: member %d at position %d is out of range, dne_set_members set members 0..%d", call, mem[i], i, set - 1);
    }
    if (!h->noise) return h->fail("noise table not uploaded (dne_noise_upload)");
    const stepenv::Dims d = se_dims(h);
    HCHECK(h, hipMemcpyAsync(h->se_io_idx, idx.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->se_io_mem, mem.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    dense::RunArgs A = dense_args(h, maze_set_members(h));
    A.idx = h->se_io_idx; A.mem = h->se_io_mem; A.B = h->se; A.max_steps = run ? max_steps : 0;
    if (run) { A.ret = h->se_io_rew; A.steps_out = h->se_io_steps; A.done_out = h->se_io_done; }
    else { A.out = h->se_io_out; A.act = h->se_io_act; }
    HCHECK(h, hipEventRecord(h->se_ev_a, h->stream));
    dense_launch(h, n, A);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->se_ev_b, h->stream));
    if (run) {
        if (reward_sum) HCHECK(h, hipMemcpyAsync(reward_sum, h->se_io_rew, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (steps_taken) HCHECK(h, hipMemcpyAsync(steps_taken, h->se_io_steps, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        if (done) HCHECK(h, hipMemcpyAsync(done, h->se_io_done, n, hipMemcpyDeviceToHost, h->stream));
    } else {
        if (out) HCHECK(h, hipMemcpyAsync(out, h->se_io_out, (size_t)n * h->dn_shape.dim[h->dn_shape.n_hidden + 1] * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (actions) HCHECK(h, hipMemcpyAsync(actions, h->se_io_act, (size_t)n * d.act * sizeof(float), hipMemcpyDeviceToHost, h->stream));   // (an int32 is a float's size)
    }
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->se_ev_a, h->se_ev_b));
    h->se_last_ms = ms;
    return 0;
}

extern "C" int dne_stepenv_act(dne_handle *h, int n, const int32_t *indices, const int32_t *members, float *out, void *actions) {
    DeviceGuard dg(h);
    return se_dense(h, "dne_stepenv_act", false, n, indices, members, 0, out, actions, nullptr, nullptr, nullptr);
}

extern "C" int dne_stepenv_run(dne_handle *h, int n, const int32_t *indices, const int32_t *members, int max_steps, float *reward_sum, int32_t *steps_taken,
                               uint8_t *done) {
    DeviceGuard dg(h);
    return se_dense(h, "dne_stepenv_run", true, n, indices, members, max_steps, nullptr, nullptr, reward_sum, steps_taken, done);
}

// the same header on the CPU: no handle, no GPU
static int dense_host_shape(const char *call, int env_kind, int n_hidden, const int32_t *widths, int nonlin, int n_out, dense::Shape *sh) {
    if (n_hidden > 0 && !widths) { g_create_error = std::string(call) + ": widths is NULL"; return -1; }
    const int nw = n_hidden < 0 ? 0 : n_hidden;   // (widths holds the n_hidden widths and nothing behind them)
    return dense_shape_error(call, dense::make_shape(env_kind, n_hidden, widths, nw, nonlin, n_out, sh), env_kind, n_hidden, widths, nw, nonlin, n_out);
}

extern "C" int dne_dense_forward_host(const float *theta, const float *obs, int n, int env_kind, int n_hidden, const int32_t *widths, int nonlin, int n_out,
                                      float *layers, float *out, void *action) {
    dense::Shape sh;
    if (dense_host_shape("dne_dense_forward_host", env_kind, n_hidden, widths, nonlin, n_out, &sh)) return -1;
    if (n < 1 || !theta || !obs || !out) { g_create_error = "dne_dense_forward_host: bad arguments"; return -1; }
    int hid = 0;
    for (int l = 1; l <= sh.n_hidden; l++) hid += sh.dim[l];
    const int act_w = env_kind == DNE_KIND_MAZE ? 2 : 1;
    for (int i = 0; i < n; i++) {
        dense::forward_host(sh, theta + (size_t)i * sh.P, obs + (size_t)i * sh.dim[0], layers ? layers + (size_t)i * hid : nullptr, out + (size_t)i * n_out);
        if (action) dense::write_action(env_kind, out + (size_t)i * n_out, (char *)action + (size_t)i * act_w * sizeof(float));
    }
    return 0;
}

extern "C" int dne_dense_rollout_host(const float *theta, int n, int env_kind, int n_hidden, const int32_t *widths, int nonlin, int n_out, const uint32_t *seeds,
                                      const double *init_state, const float *header8, const float *lines, int n_walls, int tslimit, float *returns,
                                      float *signreturns, int32_t *lengths, double *state) {
    dense::Shape sh;
    if (dense_host_shape("dne_dense_rollout_host", env_kind, n_hidden, widths, nonlin, n_out, &sh)) return -1;
    stepenv::MazeCtx mz{};
    if (se_host_args("dne_dense_rollout_host", env_kind, n, header8, lines, n_walls, &mz)) return -1;
    if (tslimit <= 0 || !theta || !returns || !lengths || !state) { g_create_error = "dne_dense_rollout_host: bad arguments"; return -1; }
    if (env_kind != DNE_KIND_MAZE && !seeds && !init_state) { g_create_error = std::string("dne_dense_rollout_host: ") + episodic_kind_name(env_kind) + " resets every environment from its seed, seeds is NULL"; return -1; }
    dense::rollout_host(sh, theta, n, seeds, init_state, mz, tslimit, returns, signreturns, lengths, state);
    return 0;
}

// ------------------------------------------------------------------------------- Deep-GA on a dense policy (csrc/dense_ga.h)
// maze_ga's bank (mzg_*: two halves of M slots and M scratch slots, the GA's own descriptors) with P = dn_shape.P at run time
static int needs_dense(dne_handle *h, const char *call) {
    return h->dense ? 0 : h->fail("%s needs a DNE_KIND_DENSE engine (this one: kind %d)", call, h->L.kind);
}

static dim3 dga_grid(dne_handle *h, int count) { return dim3(count, (h->dn_shape.P + 255) / 256); }

extern "C" int dne_dense_ga_set_init_scale(dne_handle *h, const float *scale_by, size_t n) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_ga_set_init_scale")) return -1;
    if (n != (size_t)h->dn_shape.P || !scale_by) return h->fail("dne_dense_ga_set_init_scale: expected P = %d values, got %zu", h->dn_shape.P, n);
    if (!h->mzg_mem) {
        const size_t M = h->M;
        HCHECK(h, h->alloc(&h->init_scale, n, "dense_ga_init_scale"));
        HCHECK(h, h->alloc(&h->mzg_slot, M, "dense_ga_slot")); HCHECK(h, h->alloc(&h->mzg_off, M, "dense_ga_off")); HCHECK(h, h->alloc(&h->mzg_scale, M, "dense_ga_scale"));
        float *mem = nullptr;
        HCHECK(h, h->alloc(&mem, 3 * M * h->base_stride, "dense_ga_bank"));
        HCHECK(h, hipMemset(mem, 0, 3 * M * h->base_stride * sizeof(float)));
        h->mzg_mem = mem;
    }
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(h->init_scale, scale_by, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// what every call that reads the table or the bank needs first
static int dga_ready(dne_handle *h, const char *call, bool eval) {
    if (!h->mzg_mem) return h->fail("%s: no init scale (dne_dense_ga_set_init_scale comes first)", call);
    if (!h->noise) return h->fail("%s: noise table not uploaded (dne_noise_upload)", call);
    if (eval && h->dn_shape.env == DNE_KIND_MAZE && h->maze_nw < 1) return h->fail("%s: no maze loaded (dne_maze_set_walls comes before an evaluation)", call);
    return 0;
}

extern "C" int dne_dense_ga_build(dne_handle *h, int T, const int32_t *chain_offsets, const int64_t *seeds, const float *powers) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_ga_build")) return -1;
    if (dga_ready(h, "dne_dense_ga_build", false)) return -1;
    if (T < 1 || T > h->M) return h->fail("dne_dense_ga_build: T = %d outside [1, max_members = %d]", T, h->M);
    if (!chain_offsets || !seeds || !powers) return h->fail("dne_dense_ga_build: a buffer is missing");
    if (chain_offsets[0] != 0) return h->fail("dne_dense_ga_build: chain_offsets starts at %d, not 0", chain_offsets[0]);
    const int P = h->dn_shape.P;
    const std::string bad = dense_ga::check_genomes(T, P, chain_offsets, seeds, h->noise_count);
    if (!bad.empty()) return h->fail("dne_dense_ga_build: %s", bad.c_str());
    const size_t total = (size_t)chain_offsets[T];
    if (total > h->mzg_chain_cap || !h->mzg_chain_offs) {
        HCHECK(h, hipStreamSynchronize(h->stream));
        HCHECK(h, h->release(h->mzg_chain_offs)); HCHECK(h, h->release(h->mzg_seeds)); HCHECK(h, h->release(h->mzg_powers));
        h->mzg_chain_cap = std::max<size_t>(2 * total, 4096);
        HCHECK(h, h->alloc(&h->mzg_chain_offs, (size_t)h->M + 1, "dense_ga_chain_offs"));
        HCHECK(h, h->alloc(&h->mzg_seeds, h->mzg_chain_cap, "dense_ga_seeds")); HCHECK(h, h->alloc(&h->mzg_powers, h->mzg_chain_cap, "dense_ga_powers"));
    }
    HCHECK(h, hipMemcpyAsync(h->mzg_chain_offs, chain_offsets, ((size_t)T + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->mzg_seeds, seeds, total * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->mzg_powers, powers, total * sizeof(float), hipMemcpyHostToDevice, h->stream));
    const int other = 1 - h->mzg_half;
    hipLaunchKernelGGL(dense_ga::k_dense_ga_build, dga_grid(h, T), dim3(256), 0, h->stream, (const float *)h->noise, (const float *)h->init_scale, P,
                       (const int32_t *)h->mzg_chain_offs, (const int64_t *)h->mzg_seeds, (const float *)h->mzg_powers, mzg_bank(h, other), h->base_stride);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));   // the caller's arrays may go away
    h->mzg_half = other; h->mzg_T = T;
    return 0;
}

extern "C" int dne_dense_ga_promote(dne_handle *h, int T_new, const int32_t *parent, const int64_t *idx, const float *power) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_ga_promote")) return -1;
    if (dga_ready(h, "dne_dense_ga_promote", false)) return -1;
    if (T_new < 1 || T_new > h->M) return h->fail("dne_dense_ga_promote: T = %d outside [1, max_members = %d]", T_new, h->M);
    if (!parent || !idx || !power) return h->fail("dne_dense_ga_promote: a buffer is missing");
    const int P = h->dn_shape.P;
    for (int j = 0; j < T_new; j++) {
        const std::string bad = dense_ga::check_member(j, h->mzg_T, P, h->noise_count, parent[j], idx[j], true);
        if (!bad.empty()) return h->fail("dne_dense_ga_promote: %s", bad.c_str());
    }
    if (mzg_upload_members(h, T_new, parent, idx, power)) return -1;
    const int other = 1 - h->mzg_half;
    hipLaunchKernelGGL(dense_ga::k_dense_ga_promote, dga_grid(h, T_new), dim3(256), 0, h->stream, (const float *)h->noise, (const float *)h->init_scale, P,
                       (const float *)mzg_bank(h, h->mzg_half), mzg_bank(h, other), h->base_stride, (const int32_t *)h->mzg_slot,
                       (const int64_t *)h->mzg_off, (const float *)h->mzg_scale);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->mzg_half = other; h->mzg_T = T_new;
    return 0;
}

extern "C" int dne_dense_ga_eval(dne_handle *h, int n, const int32_t *parent, const int64_t *idx, const float *power, const uint32_t *env_seed, int tslimit,
                                 float *returns, float *signreturns, int32_t *lengths) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_ga_eval")) return -1;
    if (dga_ready(h, "dne_dense_ga_eval", true)) return -1;
    if (n < 1 || n > h->M) return h->fail("dne_dense_ga_eval: n = %d outside [1, max_members = %d]", n, h->M);
    if (!parent || !idx || !power || !returns || !lengths) return h->fail("dne_dense_ga_eval: a buffer is missing");
    if (tslimit <= 0) return h->fail("dne_dense_ga_eval: timestep limit must be positive");
    if (h->dn_shape.env != DNE_KIND_MAZE && !env_seed)
        return h->fail("dne_dense_ga_eval: a DNE_KIND_DENSE engine on the %s resets every member from its environment seed, env_seed is NULL",
                       dense_env_name(h->dn_shape.env));
    // a child is k_dense_run's own member: (its parent's bank slot, idx, power); a root runs from scratch slot 2 M + i at scale 0
    const int P = h->dn_shape.P, bank0 = h->mzg_half * h->M, root0 = 2 * h->M;
    std::vector<int32_t> &slot = h->mzg_host_slot;
    std::vector<float> &scale = h->mzg_host_scale;
    slot.resize(n); scale.resize(n);
    bool roots = false;
    for (int i = 0; i < n; i++) {
        const std::string bad = dense_ga::check_member(i, h->mzg_T, P, h->noise_count, parent[i], idx[i], false);
        if (!bad.empty()) return h->fail("dne_dense_ga_eval: %s", bad.c_str());
        const bool root = parent[i] < 0;
        slot[i] = root ? root0 + i : bank0 + parent[i];
        scale[i] = root ? 0.0f : power[i];
        roots = roots || root;
    }
    if (mzg_upload_members(h, n, slot.data(), idx, scale.data())) return -1;
    if (roots) {
        hipLaunchKernelGGL(dense_ga::k_dense_ga_roots, dga_grid(h, n), dim3(256), 0, h->stream, (const float *)h->noise, (const float *)h->init_scale, P,
                           (const int32_t *)h->mzg_slot, (const int64_t *)h->mzg_off, root0, h->mzg_mem, h->base_stride);
        HCHECK(h, hipGetLastError());
    }
    return dense_eval(h, MazeMembers{h->mzg_mem, h->mzg_slot, h->mzg_off, h->mzg_scale}, "dne_dense_ga_eval", n, tslimit, env_seed, returns, signreturns,
                      lengths, nullptr);
}

extern "C" int dne_dense_ga_parents(dne_handle *h) {
    if (needs_dense(h, "dne_dense_ga_parents")) return -1;
    return h->mzg_T;
}

extern "C" int dne_dense_ga_get_parent(dne_handle *h, int j, float *out) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_ga_get_parent")) return -1;
    if (j < 0 || j >= h->mzg_T) return h->fail("dne_dense_ga_get_parent: parent %d, the bank holds %d", j, h->mzg_T);
    if (!out) return h->fail("dne_dense_ga_get_parent: no output buffer");
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipMemcpy(out, mzg_bank(h, h->mzg_half) + (size_t)j * h->base_stride, (size_t)h->dn_shape.P * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// the same header on the CPU: no handle, no GPU
static int dga_host_table(const char *call, const float *noise, size_t count, const float *scale_by, int P) {
    if (P < 1 || P > dense::MAX_P) { g_create_error = std::string(call) + ": P = " + std::to_string(P) + " outside [1, " + std::to_string(dense::MAX_P) + "]"; return -1; }
    if (!noise || !scale_by) { g_create_error = std::string(call) + ": a buffer is missing"; return -1; }
    if (count < (size_t)P) { g_create_error = std::string(call) + ": a table of " + std::to_string(count) + " floats holds no P = " + std::to_string(P) + " parameters"; return -1; }
    return 0;
}

extern "C" int dne_dense_ga_theta_host(const float *noise, size_t count, const float *scale_by, int P, const int64_t *seeds, const float *powers, int nseeds,
                                       float *out) {
    if (dga_host_table("dne_dense_ga_theta_host", noise, count, scale_by, P)) return -1;
    if (!seeds || !powers || !out) { g_create_error = "dne_dense_ga_theta_host: a buffer is missing"; return -1; }
    const int32_t co[2] = {0, nseeds};
    const std::string bad = dense_ga::check_genomes(1, P, co, seeds, count);
    if (!bad.empty()) { g_create_error = "dne_dense_ga_theta_host: " + bad; return -1; }
    dense_ga::genome_host(noise, scale_by, P, seeds, powers, nseeds, out);
    return 0;
}

extern "C" int dne_dense_ga_members_host(const float *noise, size_t count, const float *scale_by, int P, const float *bank, int T, const int32_t *parent,
                                         const int64_t *idx, const float *power, int n, float *out) {
    if (dga_host_table("dne_dense_ga_members_host", noise, count, scale_by, P)) return -1;
    if (n < 1) { g_create_error = "dne_dense_ga_members_host: n = " + std::to_string(n) + ", at least one member is needed"; return -1; }
    if (T < 0 || (T > 0 && !bank)) { g_create_error = "dne_dense_ga_members_host: T = " + std::to_string(T) + " parents without a bank"; return -1; }
    if (!parent || !idx || !power || !out) { g_create_error = "dne_dense_ga_members_host: a buffer is missing"; return -1; }
    for (int i = 0; i < n; i++) {
        const std::string bad = dense_ga::check_member(i, T, P, count, parent[i], idx[i], true);
        if (!bad.empty()) { g_create_error = "dne_dense_ga_members_host: " + bad; return -1; }
    }
    dense_ga::members_host(noise, scale_by, P, bank, parent, idx, power, n, out);
    return 0;
}

// ------------------------------------------------------------------------------- novelty over final states on a dense policy (csrc/dense_novelty.h)
// A handle is of one kind, so the archive, the host members' points and the results are the maze's fields (mzn_*) with D floats a point.
static int dnv_dim(dne_handle *h) { return dense_novelty::bc_dim(h->dn_shape.env); }

// the BCs of the last evaluation's members, formed once per evaluation (dense_eval withdraws them) on the engine's stream
static int dnv_last_bc(dne_handle *h) {
    if (h->dn_bc_valid || h->dn_last_n < 1) return 0;
    if (!h->dn_bc) HCHECK(h, h->alloc(&h->dn_bc, (size_t)h->M * dense_novelty::MAX_D, "dense_bc"));
    const int n = h->dn_last_n, env = h->dn_shape.env;
    const dim3 grid((n + 255) / 256), block(256);
    if (env == DNE_KIND_MAZE) hipLaunchKernelGGL(dense_novelty::k_dense_bc<DNE_KIND_MAZE>, grid, block, 0, h->stream, (const double *)h->dn_state, n, h->dn_bc);
    else if (env == DNE_KIND_CARTPOLE) hipLaunchKernelGGL(dense_novelty::k_dense_bc<DNE_KIND_CARTPOLE>, grid, block, 0, h->stream, (const double *)h->dn_state, n, h->dn_bc);
    else if (env == DNE_KIND_PENDULUM) hipLaunchKernelGGL(dense_novelty::k_dense_bc<DNE_KIND_PENDULUM>, grid, block, 0, h->stream, (const double *)h->dn_state, n, h->dn_bc);
    else hipLaunchKernelGGL(dense_novelty::k_dense_bc<DNE_ENV_ACROBOT>, grid, block, 0, h->stream, (const double *)h->dn_state, n, h->dn_bc);
    HCHECK(h, hipGetLastError());
    h->dn_bc_valid = true;
    return 0;
}

// bc == NULL: the last evaluation's members
static int dnv_check_members(dne_handle *h, const char *call, const float *bc, int n) {
    if (n < 1) return h->fail("%s: n = %d, at least one point is needed", call, n);
    if (!bc && n > h->dn_last_n) return h->fail("%s: %d members asked for, the last evaluation ran %d", call, n, h->dn_last_n);
    return 0;
}

extern "C" int dne_dense_bc_dim(dne_handle *h) {
    if (needs_dense(h, "dne_dense_bc_dim")) return -1;
    return dnv_dim(h);
}

extern "C" int dne_dense_bc(dne_handle *h, int n, float *bc) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_bc")) return -1;
    if (n >= 1 && n <= h->dn_last_n && bc && dnv_last_bc(h)) return -1;
    return last_eval_rows(h, "dne_dense_bc", n, h->dn_last_n, bc != nullptr, bc, (const float *)h->dn_bc, dnv_dim(h));
}

extern "C" int dne_dense_archive_append(dne_handle *h, const float *bc, int n) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_archive_append")) return -1;
    if (dnv_check_members(h, "dne_dense_archive_append", bc, n)) return -1;
    const size_t have = (size_t)h->mzn_arch_n, D = (size_t)dnv_dim(h);
    if (have + (size_t)n > (size_t)INT_MAX / 4) return h->fail("dne_dense_archive_append: %zu points would not fit an int", have + (size_t)n);
    if (mzn_reserve(h, h->mzn_arch, h->mzn_arch_cap, D * (have + n), D * have, D * MZN_ARCH_CAP0, "dense_archive")) return -1;
    if (bc) {
        HCHECK(h, hipMemcpyAsync(h->mzn_arch + D * have, bc, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HCHECK(h, hipStreamSynchronize(h->stream));   // the caller's buffer is free again
    } else {
        if (dnv_last_bc(h)) return -1;
        HCHECK(h, hipMemcpyAsync(h->mzn_arch + D * have, h->dn_bc, (size_t)n * D * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    h->mzn_arch_n += n;
    return 0;
}

extern "C" int dne_dense_archive_clear(dne_handle *h) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_archive_clear")) return -1;
    h->mzn_arch_n = 0;   // (the buffer stays; a later append lands behind every call already on the stream)
    return 0;
}

extern "C" int dne_dense_archive_size(dne_handle *h) {
    if (needs_dense(h, "dne_dense_archive_size")) return -1;
    return h->mzn_arch_n;
}

extern "C" int dne_dense_archive_get(dne_handle *h, float *bc, int cap) {
    DeviceGuard dg(h);
    if (needs_dense(h, "dne_dense_archive_get")) return -1;
    if (cap < h->mzn_arch_n) return h->fail("dne_dense_archive_get: room for %d points, the archive holds %d", cap, h->mzn_arch_n);
    if (h->mzn_arch_n > 0) {
        if (!bc) return h->fail("dne_dense_archive_get: no buffer");
        HCHECK(h, hipMemcpyAsync(bc, h->mzn_arch, (size_t)h->mzn_arch_n * dnv_dim(h) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HCHECK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

// bc staged (or the last evaluation's BCs), k_dense_novelty<D> over the kk = min(k, archive) nearest between two events, the n novelties back
extern "C" int dne_dense_novelty(dne_handle *h, const float *bc, int n, int k, double *out) {
    DeviceGuard dg(h);
    const char *call = "dne_dense_novelty";
    if (needs_dense(h, call)) return -1;
    if (dnv_check_members(h, call, bc, n)) return -1;
    if (k < 1) return h->fail("%s: k = %d, at least one neighbour is needed", call, k);
    if (k > DNE_DENSE_NOVELTY_KMAX) return h->fail("%s: k = %d, the kernel keeps at most DNE_DENSE_NOVELTY_KMAX = %d neighbours", call, k, DNE_DENSE_NOVELTY_KMAX);
    if (h->mzn_arch_n < 1) return h->fail("%s: the archive is empty (dne_dense_archive_append)", call);
    if (!out) return h->fail("%s: no output buffer", call);
    const int D = dnv_dim(h), kk = std::min(k, h->mzn_arch_n);
    const float *pts = nullptr;
    if (bc) {
        if (mzn_reserve(h, h->mzn_xy, h->mzn_xy_cap, (size_t)D * n, 0, 4096, "dense_novelty_bc")) return -1;
        HCHECK(h, hipMemcpyAsync(h->mzn_xy, bc, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice, h->stream));
        pts = h->mzn_xy;
    } else {
        if (dnv_last_bc(h)) return -1;
        pts = h->dn_bc;
    }
    if (mzn_reserve(h, h->mzn_out, h->mzn_out_cap, (size_t)n, 0, 4096, "dense_novelty_out")) return -1;
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    if (D == 2) hipLaunchKernelGGL(dense_novelty::k_dense_novelty<2>, dim3((n + 3) / 4), dim3(256), 0, h->stream, pts, n, (const float *)h->mzn_arch, h->mzn_arch_n, kk, h->mzn_out);
    else hipLaunchKernelGGL(dense_novelty::k_dense_novelty<4>, dim3((n + 3) / 4), dim3(256), 0, h->stream, pts, n, (const float *)h->mzn_arch, h->mzn_arch_n, kk, h->mzn_out);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipMemcpyAsync(out, h->mzn_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    h->mzn_last_ms = ms;
    return 0;
}

// pool novelty (GA-NS): every member against the archive and the other members, k_dense_novelty_pool<D> between two events
extern "C" int dne_dense_novelty_pool(dne_handle *h, const float *bc, int n, int k, double *out) {
    DeviceGuard dg(h);
    const char *call = "dne_dense_novelty_pool";
    if (needs_dense(h, call)) return -1;
    if (dnv_check_members(h, call, bc, n)) return -1;
    if (k < 1) return h->fail("%s: k = %d, at least one neighbour is needed", call, k);
    if (k > DNE_DENSE_NOVELTY_KMAX) return h->fail("%s: k = %d, the kernel keeps at most DNE_DENSE_NOVELTY_KMAX = %d neighbours", call, k, DNE_DENSE_NOVELTY_KMAX);
    if (h->mzn_arch_n + (n - 1) < 1) return h->fail("%s: the pool is empty (one member, no archive point)", call);
    if ((size_t)h->mzn_arch_n + (size_t)n > (size_t)INT_MAX / 4) return h->fail("%s: %zu combined slots would not fit an int", call, (size_t)h->mzn_arch_n + (size_t)n);
    if (!out) return h->fail("%s: no output buffer", call);
    const int D = dnv_dim(h), kk = std::min(k, h->mzn_arch_n + n - 1);
    const float *pts = nullptr;
    if (bc) {
        if (mzn_reserve(h, h->mzn_xy, h->mzn_xy_cap, (size_t)D * n, 0, 4096, "dense_novelty_bc")) return -1;
        HCHECK(h, hipMemcpyAsync(h->mzn_xy, bc, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice, h->stream));
        pts = h->mzn_xy;
    } else {
        if (dnv_last_bc(h)) return -1;
        pts = h->dn_bc;
    }
    if (mzn_reserve(h, h->mzn_out, h->mzn_out_cap, (size_t)n, 0, 4096, "dense_novelty_out")) return -1;
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    if (D == 2) hipLaunchKernelGGL(dense_novelty::k_dense_novelty_pool<2>, dim3((n + 3) / 4), dim3(256), 0, h->stream, pts, n, (const float *)h->mzn_arch, h->mzn_arch_n, kk, h->mzn_out);
    else hipLaunchKernelGGL(dense_novelty::k_dense_novelty_pool<4>, dim3((n + 3) / 4), dim3(256), 0, h->stream, pts, n, (const float *)h->mzn_arch, h->mzn_arch_n, kk, h->mzn_out);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipMemcpyAsync(out, h->mzn_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    h->mzn_last_ms = ms;
    return 0;
}

// archive slot A + i = the BC of the last evaluation's member members[i], device to device (k_dense_archive_gather<D>); the indices are checked
// before anything is launched, and the gather follows mzn_reserve's reallocation on the engine's stream
extern "C" int dne_dense_archive_append_members(dne_handle *h, const int32_t *members, int count) {
    DeviceGuard dg(h);
    const char *call = "dne_dense_archive_append_members";
    if (needs_dense(h, call)) return -1;
    if (count < 1) return h->fail("%s: count = %d, at least one member is needed", call, count);
    if (!members) return h->fail("%s: no member indices", call);
    for (int i = 0; i < count; i++)
        if (members[i] < 0 || members[i] >= h->dn_last_n)
            return h->fail("%s: index %d is member %d, the last evaluation ran %d", call, i, members[i], h->dn_last_n);
    const size_t have = (size_t)h->mzn_arch_n, D = (size_t)dnv_dim(h);
    if (have + (size_t)count > (size_t)INT_MAX / 4) return h->fail("%s: %zu points would not fit an int", call, have + (size_t)count);
    if (mzn_reserve(h, h->mzn_arch, h->mzn_arch_cap, D * (have + count), D * have, D * MZN_ARCH_CAP0, "dense_archive")) return -1;
    if (mzn_reserve(h, h->mzn_idx, h->mzn_idx_cap, (size_t)count, 0, 4096, "dense_archive_members")) return -1;
    if (dnv_last_bc(h)) return -1;
    HCHECK(h, hipMemcpyAsync(h->mzn_idx, members, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    const dim3 grid((count + 255) / 256), block(256);
    if (D == 2) hipLaunchKernelGGL(dense_novelty::k_dense_archive_gather<2>, grid, block, 0, h->stream, (const float *)h->dn_bc, (const int32_t *)h->mzn_idx, count, h->mzn_arch + D * have);
    else hipLaunchKernelGGL(dense_novelty::k_dense_archive_gather<4>, grid, block, 0, h->stream, (const float *)h->dn_bc, (const int32_t *)h->mzn_idx, count, h->mzn_arch + D * have);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));   // the caller's buffer is free again
    h->mzn_arch_n += count;
    return 0;
}

// the scoring kernel of the last scoring call of either form
extern "C" double dne_dense_novelty_last_ms(dne_handle *h) { return h->dense ? h->mzn_last_ms : -1.0; }

// the same header on the CPU: no handle, no GPU
extern "C" int dne_dense_novelty_host(const float *bc, int n, const float *archive, int narch, int D, int k, double *out) {
    if (!bc || !archive || !out) { g_create_error = "dne_dense_novelty_host: a buffer is missing"; return -1; }
    if (D != 2 && D != 4) { g_create_error = "dne_dense_novelty_host: D = " + std::to_string(D) + ", a behaviour characterisation has 2 or 4 values"; return -1; }
    if (n < 1) { g_create_error = "dne_dense_novelty_host: n = " + std::to_string(n) + ", at least one point is needed"; return -1; }
    if (narch < 1) { g_create_error = "dne_dense_novelty_host: the archive is empty"; return -1; }
    if (k < 1) { g_create_error = "dne_dense_novelty_host: k = " + std::to_string(k) + ", at least one neighbour is needed"; return -1; }
    dense_novelty::novelty_host(bc, n, archive, narch, D, k, out);
    return 0;
}

extern "C" int dne_dense_novelty_pool_host(const float *bc, int n, const float *archive, int narch, int D, int k, double *out) {
    if (!bc || !out || (narch > 0 && !archive)) { g_create_error = "dne_dense_novelty_pool_host: a buffer is missing"; return -1; }
    if (D != 2 && D != 4) { g_create_error = "dne_dense_novelty_pool_host: D = " + std::to_string(D) + ", a behaviour characterisation has 2 or 4 values"; return -1; }
    if (n < 1) { g_create_error = "dne_dense_novelty_pool_host: n = " + std::to_string(n) + ", at least one point is needed"; return -1; }
    if (narch < 0) { g_create_error = "dne_dense_novelty_pool_host: narch = " + std::to_string(narch); return -1; }
    if (k < 1) { g_create_error = "dne_dense_novelty_pool_host: k = " + std::to_string(k) + ", at least one neighbour is needed"; return -1; }
    if ((long long)narch + n - 1 < 1) { g_create_error = "dne_dense_novelty_pool_host: the pool is empty (one member, no archive point)"; return -1; }
    dense_novelty::novelty_pool_host(bc, n, archive, narch, D, k, out);
    return 0;
}

extern "C" int dne_dense_bc_host(int env_kind, const double *rec, int n, float *bc) {
    if (env_kind != DNE_KIND_MAZE && env_kind != DNE_KIND_CARTPOLE && env_kind != DNE_KIND_PENDULUM && env_kind != DNE_ENV_ACROBOT) {
        g_create_error = "dne_dense_bc_host: environment " + std::to_string(env_kind) + " is none of DNE_KIND_MAZE, DNE_KIND_CARTPOLE, DNE_KIND_PENDULUM, DNE_ENV_ACROBOT";
        return -1;
    }
    if (!rec || !bc) { g_create_error = "dne_dense_bc_host: a buffer is missing"; return -1; }
    if (n < 1) { g_create_error = "dne_dense_bc_host: n = " + std::to_string(n) + ", at least one record is needed"; return -1; }
    dense_novelty::bc_host(env_kind, rec, n, bc);
    return 0;
}

// ------------------------------------------------------------------------------- evaluations by descriptor: antithetic pairs, members as set
// the members set by dne_set_members through the whole-episode kernel of the engine's kind (the maze's episode is deterministic and mjmaze's has no
// reset seed: neither reads env_seed)
static int episodic_eval(dne_handle *h, const char *call, int n, int tslimit, const uint32_t *env_seed, float *returns, float *signreturns,
                         int32_t *lengths, uint8_t *bc) {
    if (h->maze) return maze_eval_members(h, maze_set_members(h), n, tslimit, returns, signreturns, lengths, bc);
    if (h->dense) return dense_eval(h, maze_set_members(h), call, n, tslimit, env_seed, returns, signreturns, lengths, bc);
    if (h->cartpole) return cartpole_eval(h, call, n, tslimit, env_seed, returns, signreturns, lengths, bc);
    if (h->pendulum) return pendulum_eval(h, maze_set_members(h), call, n, tslimit, env_seed, returns, signreturns, lengths, bc);
    return mjmaze_eval(h, maze_set_members(h), call, n, tslimit, returns, signreturns, lengths, bc);
}

extern "C" int dne_es_eval(dne_handle *h, const int64_t *idx, int n, float sigma, int tslimit, const uint32_t *env_seed,
                           float *returns_n2, float *signreturns_n2, int32_t *lengths_n2, uint8_t *bc) {
    DeviceGuard dg(h);
    // antithetic pairs over base slot 0: the ES kinds, and the GPU tree's LargeModel (its es.py runs over any model; no reference pass).
    // GAAtariPolicy's kernels take one member per group.
    if (!es_like(h->L.kind) && !h->large && !h->episodic())
        return h->fail("dne_es_eval needs an engine of kind DNE_KIND_ES, DNE_KIND_ES_VBN or DNE_KIND_GA_LARGE (this one: %d)", h->L.kind);
    if (n <= 0 || 2 * n > h->M) return h->fail("%d pairs exceed max_members = %d", n, h->M);
    std::vector<int32_t> slot(2 * n, 0);
    std::vector<int64_t> off(2 * n);
    std::vector<float> sc(2 * n);
    for (int i = 0; i < n; i++) {
        off[2 * i] = off[2 * i + 1] = idx[i];
        sc[2 * i] = sigma;        // es.py:415 params + v
        sc[2 * i + 1] = -sigma;   // es.py:419 params - v
    }
    if (dne_set_members(h, 2 * n, slot.data(), off.data(), sc.data())) return -1;
    {   // how dense the pairs lie in the stretch of the table they cover (round 6: ranks that draw from their own stretch)
        int64_t lo = idx[0], hi = idx[0];
        for (int i = 1; i < n; i++) { lo = std::min(lo, idx[i]); hi = std::max(hi, idx[i]); }
        const double span = (double)(hi - lo) + (double)h->L.P;
        h->dense_scale = std::min(16.0, std::max(1.0, (double)h->noise_count / std::max(span, 1.0)));
    }
    if (h->episodic()) return episodic_eval(h, "dne_es_eval", 2 * n, tslimit, env_seed, returns_n2, signreturns_n2, lengths_n2, bc);
    return eval_core(h, 2 * n, 2, tslimit, env_seed, returns_n2, signreturns_n2, lengths_n2, bc);
}

extern "C" int dne_eval_members(dne_handle *h, int n, int tslimit, const uint32_t *env_seed, float *returns,
                                float *signreturns, int32_t *lengths, uint8_t *bc) {
    DeviceGuard dg(h);
    if (check_n(h, n)) return -1;
    if (h->episodic()) {
        if ((int)h->host_slot.size() < n) return h->fail("dne_eval_members: %d members asked for, dne_set_members set %zu", n, h->host_slot.size());
        return episodic_eval(h, "dne_eval_members", n, tslimit, env_seed, returns, signreturns, lengths, bc);
    }
    return eval_core(h, n, 1, tslimit, env_seed, returns, signreturns, lengths, bc);
}

// ------------------------------------------------------------------------------- GA genomes
static void launch_normc(dne_handle *h, float *th) {
    const Layout &L = h->L;
    auto nc = [&](int off, int K, int C, float std) { hipLaunchKernelGGL(k_normc, dim3((C + 63) / 64), dim3(64), 0, h->stream, th + off, K, C, std); };
    auto z = [&](int off, int n) { hipLaunchKernelGGL(k_zero, dim3((n + 63) / 64), dim3(64), 0, h->stream, th + off, n); };
    nc(L.c1w, 256, 16, 1.0f); z(L.c1b, 16);
    nc(L.c2w, 256, 32, 1.0f); z(L.c2b, 32);
    nc(L.fcw, 3872, 256, 1.0f); z(L.fcb, 256);
    nc(L.ow, 256, L.nact, 0.1f); z(L.ob, L.nact);   // ac_init_std = 0.1, policies.py:434
}

// build theta(chain) into `slot`; `src_slot` >= 0 means chain[:src_len] is already materialised there
static int build_chain(dne_handle *h, int slot, const int64_t *seeds, const float *powers /*per seed or null*/, int nseeds, float sigma,
                       int src_slot, int src_len) {
    const int P = h->L.P, nb = (P + 255) / 256;
    float *dst = h->bases + (size_t)slot * h->base_stride;
    for (int s = 0; s < nseeds; s++)
        if (check_noise_range(h, seeds[s], P)) return -1;
    int start = 1;
    const float *src = dst;
    if (src_slot >= 0) {
        src = h->bases + (size_t)src_slot * h->base_stride;
        start = src_len;
        if (start == nseeds) {
            HCHECK(h, hipMemcpyAsync(dst, src, (size_t)P * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
            return 0;
        }
    } else if (powers) {   // the gpu tree's genome: root = noise[idx0] * scale_by (base.py:128-129)
        if (!h->init_scale) return h->fail("genomes with per-seed powers need dne_ga_set_init_scale first");
        const int32_t sl = slot; const int64_t o0 = seeds[0];
        int32_t *d_slot = (int32_t *)h->scratch_f;
        HCHECK(h, hipMemcpyAsync(d_slot, &sl, sizeof(sl), hipMemcpyHostToDevice, h->stream));
        HCHECK(h, hipMemcpyAsync(h->scratch_i, &o0, sizeof(o0), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_copy_noise_scaled_batch, dim3(nb, 1), dim3(256), 0, h->stream, (const float *)h->noise, (const int64_t *)h->scratch_i,
                           (const int32_t *)d_slot, h->base_stride, P, (const float *)h->init_scale, h->bases);
        HCHECK(h, hipStreamSynchronize(h->stream));   // the two scratch words are reused by the next chain
    } else {
        hipLaunchKernelGGL(k_copy_noise, dim3(nb), dim3(256), 0, h->stream, (const float *)h->noise, seeds[0], P, dst);   // ga.py:256
        launch_normc(h, dst);                                                                                                // ga.py:258-260
    }
    if (start < nseeds) {   // ga.py:262-263: all remaining mutations in one streaming pass
        const int n = nseeds - start;
        if ((size_t)n > h->chain_cap) {
            HCHECK(h, hipStreamSynchronize(h->stream));
            HCHECK(h, h->release(h->chain_offs)); HCHECK(h, h->release(h->chain_pw));
            h->chain_cap = std::max<size_t>(2 * (size_t)n, 1024);
            HCHECK(h, h->alloc(&h->chain_offs, h->chain_cap, "chain_offs")); HCHECK(h, h->alloc(&h->chain_pw, h->chain_cap, "chain_pw"));
        }
        // pageable source: the copy is staged before hipMemcpyAsync returns, so the caller's array may go away; successive
        // chains are ordered on the stream
        HCHECK(h, hipMemcpyAsync(h->chain_offs, seeds + start, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        if (powers) HCHECK(h, hipMemcpyAsync(h->chain_pw, powers + start, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_chain_sum, dim3(nb), dim3(256), 0, h->stream, (const float *)h->noise, (const int64_t *)h->chain_offs,
                           powers ? (const float *)h->chain_pw : (const float *)nullptr, n, P, sigma, src, dst);
    }
    return 0;
}

// gpu_implementation/neuroevolution/models/base.py:190-201: the per-parameter initial scale (weights std / sqrt(fan-in) in
// dqn.py:24-27, biases 0); with it set, genomes given with per-seed powers start as noise[idx0] * scale_by
extern "C" int dne_ga_set_init_scale(dne_handle *h, const float *scale_by, size_t n) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_ga_set_init_scale");
    if (es_like(h->L.kind)) return h->fail("dne_ga_set_init_scale needs a GA engine");
    if (n != (size_t)h->L.P) return h->fail("dne_ga_set_init_scale: expected %d values, got %zu", h->L.P, n);
    if (!h->init_scale) HCHECK(h, h->alloc(&h->init_scale, n, "init_scale"));
    HCHECK(h, hipMemcpy(h->init_scale, scale_by, n * sizeof(float), hipMemcpyHostToDevice));
    h->ga_cache.clear();
    h->child_slots.clear();          // every slot but 0 is free again -- including the ones set aside for materialised children
    h->free_slots.clear();
    for (int s2 = h->base_cap - 1; s2 >= 1; s2--) h->free_slots.push_back(s2);
    return 0;
}

extern "C" int dne_ga_rebuild(dne_handle *h, int slot, const int64_t *seeds, int nseeds, float sigma, float *out_host) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_ga_rebuild");
    if (h->L.kind != DNE_KIND_GA) return h->fail("dne_ga_rebuild needs a GAAtariPolicy engine (LargeModel genomes carry per-seed powers: dne_ga_rebuild_powers)");
    if (slot < 0 || nseeds < 1) return h->fail("bad arguments");
    if (grow_bases(h, slot + 1)) return -1;
    claim_slot(h, slot);
    if (build_chain(h, slot, seeds, nullptr, nseeds, sigma, -1, 0)) return -1;
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (out_host) HCHECK(h, hipMemcpy(out_host, h->bases + (size_t)slot * h->base_stride, (size_t)h->L.P * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// the same for a genome ((idx0,), (idx1, power1), ...) of the gpu tree (base.py:118-139: compute_weights_from_seeds)
extern "C" int dne_ga_rebuild_powers(dne_handle *h, int slot, const int64_t *seeds, const float *powers, int nseeds, float *out_host) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_ga_rebuild_powers");
    if (es_like(h->L.kind)) return h->fail("dne_ga_rebuild_powers needs a GA engine");
    if (slot < 0 || nseeds < 1 || !powers) return h->fail("bad arguments");
    if (grow_bases(h, slot + 1)) return -1;
    claim_slot(h, slot);
    if (build_chain(h, slot, seeds, powers, nseeds, 0.0f, -1, 0)) return -1;
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (out_host) HCHECK(h, hipMemcpy(out_host, h->bases + (size_t)slot * h->base_stride, (size_t)h->L.P * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// Every child = parent chain + one fresh seed (ga.py:251-254).  Parents are materialised once into base slots (cached
// across generations by chain) and the child's last mutation is applied on the fly by the forward kernels, exactly like an
// ES perturbation with scale +sigma.  powers == null: es_distributed genomes (normc root, one sigma); powers != null: the
// gpu tree's genomes ((idx0,), (idx1, power1), ...) with a scaled-noise root (base.py:118-149).
static int ga_eval_impl(dne_handle *h, const int32_t *co, const int64_t *seeds, const float *powers, int n, float sigma, int tslimit,
                        const uint32_t *env_seed, float *returns, float *signreturns, int32_t *lengths, uint8_t *bc) {
    if (es_like(h->L.kind)) return h->fail("dne_ga_eval needs a GA engine");
    if (h->large && !powers) return h->fail("LargeModel genomes are the GPU tree's: per-seed powers over a scaled-noise root (dne_ga_set_init_scale + dne_ga_eval_powers)");
    if (check_n(h, n)) return -1;
    if (powers && !h->init_scale) return h->fail("genomes with per-seed powers need dne_ga_set_init_scale first");
    const int stride = powers ? 2 : 1;   // cache key: the seeds, interleaved with the bit patterns of their powers
    const int mode = powers ? 2 : 1;
    auto key_of = [&](const int64_t *c, const float *pw, int len) {
        std::vector<int64_t> k((size_t)len * stride);
        for (int j = 0; j < len; j++) {
            k[(size_t)j * stride] = c[j];
            if (powers) { uint32_t bits = 0; if (j > 0) memcpy(&bits, &pw[j], 4); k[(size_t)j * stride + 1] = (int64_t)bits; }
        }
        return k;
    };
    std::vector<std::vector<int64_t>> prefix(n);
    std::vector<int64_t> off(n);
    std::vector<float> sc(n);
    std::map<std::vector<int64_t>, int> needed;
    for (int i = 0; i < n; i++) {
        const int len = co[i + 1] - co[i];
        if (len < 1) return h->fail("member %d has an empty seed chain", i);
        const int64_t *c = seeds + co[i];
        for (int j = 0; j < len; j++)
            if (check_noise_range(h, c[j], h->L.P)) return -1;
        const float *pw = powers ? powers + co[i] : nullptr;
        if (len == 1) { prefix[i] = key_of(c, pw, 1); off[i] = c[0]; sc[i] = 0.0f; }
        else { prefix[i] = key_of(c, pw, len - 1); off[i] = c[len - 1]; sc[i] = powers ? pw[len - 1] : sigma; }
        needed[prefix[i]] = -1;
    }
    // (only now: a call refused above leaves the store as it was)
    if (h->ga_cache_mode != mode || (!powers && h->ga_cache_sigma != sigma)) {   // cached parents were built under other rules
        for (auto &kv : h->ga_cache) h->free_slots.push_back(kv.second);
        h->ga_cache.clear();
        h->ga_cache_mode = mode; h->ga_cache_sigma = sigma;
    }
    size_t fresh = 0;
    for (auto &kv : needed) fresh += h->ga_cache.count(kv.first) ? 0 : 1;
    if (fresh > h->free_slots.size()) {
        if (grow_bases(h, h->base_cap + (int)(fresh - h->free_slots.size()))) return -1;
    }
    struct Fresh { const std::vector<int64_t> *chain; int slot, src_slot, src_len; };
    std::vector<Fresh> fresh_list;
    for (auto &kv : needed) {
        auto it = h->ga_cache.find(kv.first);
        if (it != h->ga_cache.end()) { kv.second = it->second; continue; }
        const int slot = h->free_slots.back();
        h->free_slots.pop_back();
        // longest cached proper prefix as the starting point
        int src_slot = -1, src_len = 0;
        std::vector<int64_t> p(kv.first);
        while ((int)p.size() > stride) {
            p.resize(p.size() - stride);
            auto jt = h->ga_cache.find(p);
            if (jt != h->ga_cache.end()) { src_slot = jt->second; src_len = (int)p.size() / stride; break; }
        }
        kv.second = slot;
        fresh_list.push_back({&kv.first, slot, src_slot, src_len});
    }
    {   // genomes with no cached ancestor: one batched launch set for all roots.  es_distributed: normc(noise[s0])
        // (ga.py:256-260); gpu tree: noise[s0] * scale_by (base.py:128-129)
        std::vector<int32_t> rslot; std::vector<int64_t> roff;
        for (auto &f : fresh_list)
            if (f.src_slot < 0) {
                if (check_noise_range(h, (*f.chain)[0], h->L.P)) return -1;
                rslot.push_back(f.slot); roff.push_back((*f.chain)[0]);
            }
        const int nr = (int)rslot.size();
        if (nr > 0) {
            if (scratch_reserve(h, (size_t)nr)) return -1;
            int32_t *d_slot = (int32_t *)h->scratch_f;
            HCHECK(h, hipMemcpyAsync(d_slot, rslot.data(), nr * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HCHECK(h, hipMemcpyAsync(h->scratch_i, roff.data(), nr * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
            const Layout &L = h->L;
            const size_t st = h->base_stride;
            if (powers) {
                hipLaunchKernelGGL(k_copy_noise_scaled_batch, dim3((L.P + 255) / 256, nr), dim3(256), 0, h->stream, (const float *)h->noise,
                                   (const int64_t *)h->scratch_i, (const int32_t *)d_slot, st, L.P, (const float *)h->init_scale, h->bases);
            } else {
                hipLaunchKernelGGL(k_copy_noise_batch, dim3((L.P + 255) / 256, nr), dim3(256), 0, h->stream, (const float *)h->noise,
                                   (const int64_t *)h->scratch_i, (const int32_t *)d_slot, st, L.P, h->bases);
                auto nc = [&](int off, int K, int C, float sd) { hipLaunchKernelGGL(k_normc_batch, dim3((C + 63) / 64, nr), dim3(64), 0, h->stream, h->bases, (const int32_t *)d_slot, st, off, K, C, sd); };
                auto z = [&](int off, int n2) { hipLaunchKernelGGL(k_zero_batch, dim3((n2 + 63) / 64, nr), dim3(64), 0, h->stream, h->bases, (const int32_t *)d_slot, st, off, n2); };
                nc(L.c1w, 256, 16, 1.0f); z(L.c1b, 16);
                nc(L.c2w, 256, 32, 1.0f); z(L.c2b, 32);
                nc(L.fcw, 3872, 256, 1.0f); z(L.fcb, 256);
                nc(L.ow, 256, L.nact, 0.1f); z(L.ob, L.nact);
            }
            HCHECK(h, hipStreamSynchronize(h->stream));   // scratch is reused below
        }
    }
    std::vector<int64_t> cs; std::vector<float> cp;
    for (auto &f : fresh_list) {
        const auto &key = *f.chain;
        const int len = (int)key.size() / stride;
        cs.resize(len); cp.resize(len);
        for (int j = 0; j < len; j++) {
            cs[j] = key[(size_t)j * stride];
            if (powers) { const uint32_t bits = (uint32_t)key[(size_t)j * stride + 1]; memcpy(&cp[j], &bits, 4); }
        }
        const float *pw = powers ? cp.data() : nullptr;
        if (f.src_slot < 0) {   // root already initialised; apply the remaining mutations in place
            if (len > 1 && build_chain(h, f.slot, cs.data(), pw, len, sigma, f.slot, 1)) return -1;
        } else if (build_chain(h, f.slot, cs.data(), pw, len, sigma, f.src_slot, f.src_len)) return -1;
        HCHECK(h, hipStreamSynchronize(h->stream));   // cs / cp are reused by the next chain
    }
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    // keep only this generation's parents cached
    for (auto it = h->ga_cache.begin(); it != h->ga_cache.end();) {
        if (!needed.count(it->first)) { h->free_slots.push_back(it->second); it = h->ga_cache.erase(it); }
        else ++it;
    }
    for (auto &kv : needed) h->ga_cache[kv.first] = kv.second;
    std::vector<int32_t> slot(n);
    for (int i = 0; i < n; i++) slot[i] = needed[prefix[i]];
    // Children of one parent sit next to each other in the member order (DNE_GA_SORT=0 keeps the caller's order): the workgroups
    // that run side by side then stream the same parent rows, which the L2 serves once.  Members are independent, so the results
    // are the same in any order; they are handed back in the caller's.
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    if (h->k.ga_sort) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return slot[a] < slot[b]; });
    std::vector<int32_t> pslot(n); std::vector<int64_t> poff(n); std::vector<float> psc(n); std::vector<uint32_t> pseed(n);
    for (int j = 0; j < n; j++) { const int i = order[j]; pslot[j] = slot[i]; poff[j] = off[i]; psc[j] = sc[i]; pseed[j] = env_seed[i]; }
    h->members_materialized = false;
    if (h->k.ga_materialize) {
        // Every child's vector written out once (parent + power * noise, the forward kernels' own two roundings): a member-step then
        // reads its rows as they are instead of streaming a parent row and a noise row -- for the LargeModel, whose 20 parents
        // (318 MB) do not fit the Infinity Cache, half the HBM bytes of the fc.  Roots (no mutation) are their own vector already.
        if (h->child_slots.size() < (size_t)n) {
            const int need = n - (int)h->child_slots.size();
            if ((int)h->free_slots.size() < need && grow_bases(h, h->base_cap + need - (int)h->free_slots.size())) return -1;
            for (int k = 0; k < need; k++) { h->child_slots.push_back(h->free_slots.back()); h->free_slots.pop_back(); }
        }
        std::vector<int32_t> cs(n), mp; std::vector<int64_t> mo; std::vector<float> ms; std::vector<int32_t> mc;
        for (int j = 0; j < n; j++) {
            if (psc[j] == 0.0f) { cs[j] = pslot[j]; continue; }
            cs[j] = h->child_slots[j];
            mp.push_back(pslot[j]); mo.push_back(poff[j]); ms.push_back(psc[j]); mc.push_back(cs[j]);
        }
        const int nm = (int)mp.size();
        if (nm > 0) {
            if (scratch_reserve(h, (size_t)3 * nm)) return -1;
            int32_t *d_ps = (int32_t *)h->scratch_f, *d_cs = d_ps + nm;
            float *d_sc = h->scratch_f + 2 * nm;
            HCHECK(h, hipMemcpyAsync(d_ps, mp.data(), nm * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HCHECK(h, hipMemcpyAsync(d_cs, mc.data(), nm * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HCHECK(h, hipMemcpyAsync(d_sc, ms.data(), nm * sizeof(float), hipMemcpyHostToDevice, h->stream));
            HCHECK(h, hipMemcpyAsync(h->scratch_i, mo.data(), nm * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_materialize_children, dim3((h->L.P + 255) / 256, nm), dim3(256), 0, h->stream, (const float *)h->noise, h->bases,
                               h->base_stride, h->L.P, (const int32_t *)d_ps, (const int64_t *)h->scratch_i, (const float *)d_sc, (const int32_t *)d_cs);
            HCHECK(h, hipStreamSynchronize(h->stream));
        }
        for (int j = 0; j < n; j++) { pslot[j] = cs[j]; psc[j] = 0.0f; }
    }
    if (dne_set_members(h, n, pslot.data(), poff.data(), psc.data())) return -1;
    h->members_materialized = h->k.ga_materialize != 0;   // (dne_set_members clears it: a caller's own members carry noise)
    h->host_caller.assign(order.begin(), order.end());
    std::vector<float> pret(n), psg(n); std::vector<int32_t> plen(n); std::vector<uint8_t> pbc(bc ? (size_t)n * 128 : 0);
    if (eval_core(h, n, 1, tslimit, pseed.data(), pret.data(), psg.data(), plen.data(), bc ? pbc.data() : nullptr)) return -1;
    if (h->ram_last_n == n) h->ram_last_caller.assign(order.begin(), order.end());
    for (int j = 0; j < n; j++) {
        const int i = order[j];
        returns[i] = pret[j]; lengths[i] = plen[j];
        if (signreturns) signreturns[i] = psg[j];
        if (bc) memcpy(bc + (size_t)i * 128, pbc.data() + (size_t)j * 128, 128);
    }
    return 0;
}

extern "C" int dne_ga_eval(dne_handle *h, const int32_t *co, const int64_t *seeds, int n, float sigma, int tslimit,
                           const uint32_t *env_seed, float *returns, float *signreturns, int32_t *lengths, uint8_t *bc) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_ga_eval");
    return ga_eval_impl(h, co, seeds, nullptr, n, sigma, tslimit, env_seed, returns, signreturns, lengths, bc);
}

// gpu_implementation/ga.py:161-166: offspring ((idx0,), (idx1, power1), ...) -- powers[] runs parallel to seeds[] (the root's
// entry is ignored); needs dne_ga_set_init_scale
extern "C" int dne_ga_eval_powers(dne_handle *h, const int32_t *co, const int64_t *seeds, const float *powers, int n, int tslimit,
                                  const uint32_t *env_seed, float *returns, float *signreturns, int32_t *lengths, uint8_t *bc) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_ga_eval_powers");
    if (!powers) return h->fail("dne_ga_eval_powers: powers missing");
    return ga_eval_impl(h, co, seeds, powers, n, 0.0f, tslimit, env_seed, returns, signreturns, lengths, bc);
}

// ------------------------------------------------------------------------------- reduce
extern "C" int dne_centered_ranks(dne_handle *h, const float *x, int n, float *out) {
    DeviceGuard dg(h);
    if (n < 2) return h->fail("dne_centered_ranks: n = %d unsupported", n);
    if (rec_reserve(h, (n + 1) / 2, 1)) return -1;
    HCHECK(h, hipMemcpyAsync(h->scratch_f, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_centered_ranks, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const float *)h->scratch_f, n, h->scratch_f + n);
    HCHECK(h, hipMemcpyAsync(out, h->scratch_f + n, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

static int weighted_sum_dev(dne_handle *h, const int64_t *idx_host, const float *w_dev, int n, float denom) {
    for (int i = 0; i < n; i++)
        if (check_noise_range(h, idx_host[i], h->L.P)) return -1;
    HCHECK(h, hipMemcpyAsync(h->scratch_i, idx_host, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    hipLaunchKernelGGL(k_weighted_sum, dim3((h->L.P + 255) / 256), dim3(256), 0, h->stream, (const float *)h->noise,
                       (const int64_t *)h->scratch_i, w_dev, n, h->L.P, denom, h->g);
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    h->prof.reduce_ms = ms;
    return 0;
}

extern "C" int dne_weighted_sum(dne_handle *h, const int64_t *idx, const float *w, int n, float denom, float *g_host) {
    DeviceGuard dg(h);
    if (n < 1) return h->fail("dne_weighted_sum: n = %d unsupported", n);
    if (rec_reserve(h, n, 1)) return -1;
    HCHECK(h, hipMemcpyAsync(h->scratch_f, w, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (weighted_sum_dev(h, idx, h->scratch_f, n, denom)) return -1;
    if (g_host) HCHECK(h, hipMemcpy(g_host, h->g, (size_t)h->L.P * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int dne_optimizer_reset(dne_handle *h) {
    DeviceGuard dg(h);
    HCHECK(h, hipMemsetAsync(h->opt_m, 0, h->L.P * sizeof(float), h->stream));
    HCHECK(h, hipMemsetAsync(h->opt_v, 0, h->L.P * sizeof(float), h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->opt_t = 0;
    return 0;
}

extern "C" int dne_optimizer_get_state(dne_handle *h, float *m, float *v, int32_t *t) {
    DeviceGuard dg(h);
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (m) HCHECK(h, hipMemcpy(m, h->opt_m, (size_t)h->L.P * sizeof(float), hipMemcpyDeviceToHost));
    if (v) HCHECK(h, hipMemcpy(v, h->opt_v, (size_t)h->L.P * sizeof(float), hipMemcpyDeviceToHost));
    if (t) *t = h->opt_t;
    return 0;
}

extern "C" int dne_optimizer_set_state(dne_handle *h, const float *m, const float *v, int32_t t) {
    DeviceGuard dg(h);
    if (t < 0) return h->fail("optimizer step count must be >= 0");
    // optimizers.py:11 adds one before the step: the largest int32 would overflow there
    if (t == INT32_MAX) return h->fail("dne_optimizer_set_state: t = %d leaves no room for the next step (the count is an int32)", t);
    if (m) HCHECK(h, hipMemcpy(h->opt_m, m, (size_t)h->L.P * sizeof(float), hipMemcpyHostToDevice));
    if (v) HCHECK(h, hipMemcpy(h->opt_v, v, (size_t)h->L.P * sizeof(float), hipMemcpyHostToDevice));
    h->opt_t = t;
    return 0;
}

extern "C" int dne_optimizer_step(dne_handle *h, int kind, float l2, double stepsize, double b1m, double b2, double eps,
                                  double *ratio) {
    DeviceGuard dg(h);
    const int P = h->L.P, nb = (P + 255) / 256;
    h->opt_t += 1;   // optimizers.py:11
    if (kind == DNE_OPT_ADAM) {
        const double a = stepsize * std::sqrt(1.0 - std::pow(b2, (double)h->opt_t)) / (1.0 - std::pow(b1m, (double)h->opt_t));
        hipLaunchKernelGGL(k_adam, dim3(nb), dim3(256), 0, h->stream, h->bases, h->opt_m, h->opt_v, (const float *)h->g, P, l2,
                           (float)(-a), (float)b1m, (float)(1.0 - b1m), (float)b2, (float)(1.0 - b2), (float)eps, h->partial);
    } else if (kind == DNE_OPT_SGD) {
        hipLaunchKernelGGL(k_sgd, dim3(nb), dim3(256), 0, h->stream, h->bases, h->opt_v, (const float *)h->g, P, l2, (float)b1m,
                           (float)(1.0 - b1m), (float)(-stepsize), h->partial);
    } else {
        return h->fail("unknown optimizer kind %d", kind);
    }
    HCHECK(h, hipGetLastError());
    std::vector<double> part(2 * (size_t)nb);
    HCHECK(h, hipMemcpyAsync(part.data(), h->partial, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    double ss = 0, tt = 0;
    for (int b = 0; b < nb; b++) { ss += part[2 * b]; tt += part[2 * b + 1]; }
    if (ratio) *ratio = std::sqrt(ss) / std::sqrt(tt);
    return 0;
}

// ------------------------------------------------------------------------------- exchange
// One generation's per-pair records, gathered from every GPU, live on the device in global pair order
// (rec_idx / rec_ret / rec_sign / rec_len) and feed the update directly.
static int rec_reserve(dne_handle *h, int n_global, int per_world) {
    if ((size_t)n_global > h->rec_cap) {
        HCHECK(h, h->release(h->rec_idx)); HCHECK(h, h->release(h->rec_ret)); HCHECK(h, h->release(h->rec_sign));
        HCHECK(h, h->release(h->rec_len));
        const size_t cap = std::max<size_t>((size_t)n_global, 4096);
        HCHECK(h, h->alloc(&h->rec_idx, cap, "rec_idx")); HCHECK(h, h->alloc(&h->rec_ret, 2 * cap, "rec_ret"));
        HCHECK(h, h->alloc(&h->rec_sign, 2 * cap, "rec_sign")); HCHECK(h, h->alloc(&h->rec_len, 2 * cap, "rec_len"));
        h->rec_cap = cap;
    }
    // wire buffers: send = one shard, recv = all shards (padded to equal size), + the ordered copy for the host
    const size_t wire = (size_t)std::max(per_world, n_global) * sizeof(PairRecord);
    if (wire > h->rec_wire_cap) {
        HCHECK(h, h->release(h->rec_send)); HCHECK(h, h->release(h->rec_recv));
        HCHECK(h, h->alloc(&h->rec_send, wire, "rec_send")); HCHECK(h, h->alloc(&h->rec_recv, 2 * wire, "rec_recv"));
        h->rec_wire_cap = wire;
    }
    // scratch for processed returns [2N] + raw copy [2N] + weights [N]
    return scratch_reserve(h, (size_t)5 * n_global + 64);
}

struct Rccl {   // the few entry points of librccl.so the exchange needs
    ncclResult_t (*GetUniqueId)(ncclUniqueId *);
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    ncclResult_t (*CommAbort)(ncclComm_t);
    ncclResult_t (*CommCount)(const ncclComm_t, int *);
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *);
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    const char *(*GetErrorString)(ncclResult_t);
    void *lib = nullptr;
};
static Rccl g_rccl;

static const char *rccl_open() {   // nullptr on success, else the reason
    if (g_rccl.lib) return nullptr;
    void *lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return dlerror();
#define SYM(field, name) do { *(void **)&g_rccl.field = dlsym(lib, name); if (!g_rccl.field) return "librccl.so.1 lacks " name; } while (0)
    SYM(GetUniqueId, "ncclGetUniqueId"); SYM(CommInitRank, "ncclCommInitRank"); SYM(CommDestroy, "ncclCommDestroy");
    SYM(CommAbort, "ncclCommAbort"); SYM(CommCount, "ncclCommCount"); SYM(CommUserRank, "ncclCommUserRank");
    SYM(AllGather, "ncclAllGather"); SYM(AllReduce, "ncclAllReduce"); SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    g_rccl.lib = lib;
    return nullptr;
}
#define NCHECK(h, expr)                                                                                   \
    do {                                                                                                  \
        ncclResult_t _r = (expr);                                                                         \
        if (_r != ncclSuccess) return (h)->fail("%s:%d %s -> %s", __FILE__, __LINE__, #expr, g_rccl.GetErrorString(_r)); \
    } while (0)

extern "C" int dne_comm_unique_id(void *out128) {
    if (const char *why = rccl_open()) { g_create_error = std::string("dne_comm_unique_id: cannot open librccl.so.1: ") + why; return -1; }
    ncclUniqueId id;
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return -1; }
    memcpy(out128, &id, sizeof(id));
    return 0;
}

extern "C" int dne_comm_init(dne_handle *h, int rank, int nranks, const void *unique_id128) {
    DeviceGuard dg(h);
    if (nranks < 1 || rank < 0 || rank >= nranks) return h->fail("dne_comm_init: rank %d of %d", rank, nranks);
    if (h->comm) return h->fail("dne_comm_init: communicator already initialised");
    if (const char *why = rccl_open()) return h->fail("dne_comm_init: cannot open librccl.so.1: %s", why);
    ncclUniqueId id;
    memcpy(&id, unique_id128, sizeof(id));
    ncclComm_t c = nullptr;
    h->trace("comm init: rank %d of %d", rank, nranks);
    // the one call that can block for long (a peer that never arrives).  If the caller has meanwhile given up (dne_comm_abort from
    // the thread that owns the handle), that thread is using the handle: from here on this late path touches NOTHING of it but the
    // atomic flag -- no error text (h->fail writes the shared buffer), no trace -- and returns a code.  The handle must not be
    // destroyed while an initialisation is still in flight (bench.py leaves through os._exit in that case).
    const ncclResult_t init_rc = g_rccl.CommInitRank(&c, nranks, id, rank);
    {   // the flag is read and the communicator published under the lock dne_comm_abort takes: an abort either comes first (this
        // call drops its communicator) or finds the published one and aborts it -- never a live communicator on a handle that is off
        std::lock_guard<std::mutex> lk(h->comm_mu);
        if (h->comm_off.load(std::memory_order_acquire)) {
            if (init_rc == ncclSuccess && c) g_rccl.CommAbort(c);
            return -2;   // DNE_COMM_DROPPED
        }
        if (init_rc == ncclSuccess) { h->comm = c; h->comm_rank = rank; h->comm_size = nranks; }
    }
    if (init_rc != ncclSuccess) return h->fail("ncclCommInitRank -> %s", g_rccl.GetErrorString(init_rc));
    HCHECK(h, h->alloc(&h->comm_scratch, 64, "comm_scratch"));
    h->trace("comm ready");
    return 0;
}

extern "C" int dne_comm_info(dne_handle *h, int *rank, int *nranks, int *is_rccl) {
    int r = 0, n = 1;
    if (h->comm) {
        NCHECK(h, g_rccl.CommUserRank((ncclComm_t)h->comm, &r));
        NCHECK(h, g_rccl.CommCount((ncclComm_t)h->comm, &n));
    }
    if (rank) *rank = r;
    if (nranks) *nranks = n;
    if (is_rccl) *is_rccl = h->comm ? 1 : 0;
    return 0;
}

extern "C" int dne_device_count(int *count) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess && e != hipErrorNoDevice) { g_create_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return -1; }
    *count = e == hipSuccess ? n : 0;
    return 0;
}

static void comm_destroy(dne_handle *h) {
    if (h->comm && !h->comm_borrowed) g_rccl.CommDestroy((ncclComm_t)h->comm);
    h->comm = nullptr;
}

// Several engines of one process (one per workload, all on the same device) take part in the collectives of one communicator:
// `h` borrows the communicator `owner` built with dne_comm_init.  The calls of a process are issued by one host thread, engine
// after engine, so their order is the same on every rank; the owner must outlive the borrower's last collective.
extern "C" int dne_comm_share(dne_handle *h, dne_handle *owner) {
    if (!owner || !owner->comm) return h->fail("dne_comm_share: the other handle has no communicator");
    if (h->comm) return h->fail("dne_comm_share: communicator already initialised");
    if (h->cfg.device_id != owner->cfg.device_id) return h->fail("dne_comm_share: the two handles are on different devices");
    DeviceGuard dg(h);
    h->comm = owner->comm; h->comm_rank = owner->comm_rank; h->comm_size = owner->comm_size; h->comm_borrowed = true;
    HCHECK(h, h->alloc(&h->comm_scratch, 64, "comm_scratch"));
    return 0;
}

// Give up on RCCL for this handle (the ranks agreed on another carrier): an existing communicator is aborted, one that a
// still-running dne_comm_init on another thread produces later is dropped.  Afterwards the handle behaves like a single rank.
extern "C" int dne_comm_abort(dne_handle *h) {
    std::lock_guard<std::mutex> lk(h->comm_mu);
    h->comm_off.store(true, std::memory_order_release);
    if (h->comm && !h->comm_borrowed && g_rccl.lib) g_rccl.CommAbort((ncclComm_t)h->comm);
    h->comm = nullptr; h->comm_rank = 0; h->comm_size = 1;
    return 0;
}

// element-wise sum (op 0) or max (op 1) of n <= 64 doubles over all ranks; with n = 0 it is the barrier of bench.py
extern "C" int dne_comm_allreduce(dne_handle *h, double *inout, int n, int op) {
    DeviceGuard dg(h);
    if (n < 0 || n > 64 || (op != 0 && op != 1)) return h->fail("dne_comm_allreduce: bad arguments");
    if (!h->comm) {   // a single rank: nothing to combine
        HCHECK(h, hipDeviceSynchronize());
        return 0;
    }
    const int cnt = std::max(n, 1);
    double zero = 0.0;
    HCHECK(h, hipMemcpyAsync(h->comm_scratch, n ? inout : &zero, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
    NCHECK(h, g_rccl.AllReduce(h->comm_scratch, h->comm_scratch, cnt, ncclDouble, op == 0 ? ncclSum : ncclMax, (ncclComm_t)h->comm, h->stream));
    if (n) HCHECK(h, hipMemcpyAsync(inout, h->comm_scratch, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    HCHECK(h, hipDeviceSynchronize());
    return 0;
}

// generic small all-gather (the GA's child records, ga.py:266-271 Results): every rank contributes `bytes` bytes from the
// host and receives nranks * bytes in rank order; staged through the wire buffers, RCCL on the engine's stream
extern "C" int dne_comm_allgather(dne_handle *h, const void *send, size_t bytes, void *recv) {
    DeviceGuard dg(h);
    if (!bytes) return 0;
    if (!h->comm) { memcpy(recv, send, bytes); return 0; }
    const size_t world = (size_t)h->comm_size;
    const int as_pairs = (int)((bytes * world + sizeof(PairRecord) - 1) / sizeof(PairRecord));
    if (rec_reserve(h, 1, as_pairs)) return -1;   // wire buffers: send >= bytes, recv >= world * bytes
    HCHECK(h, hipMemcpyAsync(h->rec_send, send, bytes, hipMemcpyHostToDevice, h->stream));
    NCHECK(h, g_rccl.AllGather(h->rec_send, h->rec_recv, bytes, ncclChar, (ncclComm_t)h->comm, h->stream));
    HCHECK(h, hipMemcpyAsync(recv, h->rec_recv, bytes * world, hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

static int check_records_host(dne_handle *h, int n_global) {
    for (int i = 0; i < n_global; i++)
        if (check_noise_range(h, h->rec_idx_host[i], h->L.P)) return -1;
    return 0;
}

// this rank's shard of the last dne_es_eval as wire records (for transports other than RCCL: the redis Result path,
// the gloo tests)
extern "C" int dne_records_pack(dne_handle *h, int n_local, void *records_out) {
    DeviceGuard dg(h);
    if ((!es_like(h->L.kind) && !h->large && !h->episodic()) || n_local < 1 || 2 * n_local > h->M) return h->fail("dne_records_pack: %d pairs", n_local);
    if (rec_reserve(h, n_local, n_local)) return -1;
    hipLaunchKernelGGL(k_records_pack, dim3((n_local + 255) / 256), dim3(256), 0, h->stream, (const int64_t *)h->m_off, (const float *)h->ret,
                       (const float *)h->sign, (const int32_t *)h->len, n_local, n_local, (PairRecord *)h->rec_send);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipMemcpyAsync(records_out, h->rec_send, (size_t)n_local * sizeof(PairRecord), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// gathered records from the host (global pair order) -> device-resident, ready for dne_es_update_gathered
extern "C" int dne_records_set(dne_handle *h, const void *records, int n_global) {
    DeviceGuard dg(h);
    if (n_global < 1) return h->fail("dne_records_set: %d pairs", n_global);
    if (rec_reserve(h, n_global, n_global)) return -1;
    HCHECK(h, hipMemcpyAsync(h->rec_recv, records, (size_t)n_global * sizeof(PairRecord), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_records_unpack, dim3((n_global + 255) / 256), dim3(256), 0, h->stream, (const PairRecord *)h->rec_recv, n_global, 1,
                       n_global, h->rec_idx, h->rec_ret, h->rec_sign, h->rec_len, (PairRecord *)nullptr);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    const PairRecord *r = (const PairRecord *)records;
    h->rec_idx_host.resize(n_global);
    for (int i = 0; i < n_global; i++) h->rec_idx_host[i] = r[i].noise_idx;
    h->rec_n = n_global;
    return check_records_host(h, n_global);
}

// The exchange step of a generation: every rank contributes the records of the n_local pairs it just evaluated
// (global pairs rank, rank + world, ...) straight from its device accumulators; one RCCL all-gather over xGMI; the
// result stays on the device in global pair order.  records_out (n_global x 32 bytes, may be NULL) receives a host copy
// for logging.  Without a communicator (one GPU) it is a local repack.
extern "C" int dne_allgather_results(dne_handle *h, int n_local, int n_global, void *records_out) {
    DeviceGuard dg(h);
    const int world = h->comm ? h->comm_size : 1, rank = h->comm ? h->comm_rank : 0;
    if (!es_like(h->L.kind) && !h->large && !h->episodic()) return h->fail("dne_allgather_results needs an engine dne_es_eval accepts (DNE_KIND_ES, DNE_KIND_ES_VBN, DNE_KIND_GA_LARGE)");
    const int mine = n_global > rank ? (n_global - rank + world - 1) / world : 0;
    if (n_global < 1 || n_local != mine || 2 * n_local > h->M)
        return h->fail("dne_allgather_results: rank %d of %d holds %d pairs, a population of %d pairs gives it %d", rank, world, n_local, n_global, mine);
    const int per = (n_global + world - 1) / world;
    if (rec_reserve(h, n_global, per * world)) return -1;
    hipLaunchKernelGGL(k_records_pack, dim3((per + 255) / 256), dim3(256), 0, h->stream, (const int64_t *)h->m_off, (const float *)h->ret,
                       (const float *)h->sign, (const int32_t *)h->len, n_local, per, (PairRecord *)h->rec_send);
    PairRecord *gathered = (PairRecord *)h->rec_recv, *ordered = gathered + (size_t)per * world;
    if (world > 1) NCHECK(h, g_rccl.AllGather(h->rec_send, gathered, (size_t)per * sizeof(PairRecord), ncclChar, (ncclComm_t)h->comm, h->stream));
    else HCHECK(h, hipMemcpyAsync(gathered, h->rec_send, (size_t)per * sizeof(PairRecord), hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(k_records_unpack, dim3((n_global + 255) / 256), dim3(256), 0, h->stream, (const PairRecord *)gathered, n_global, world,
                       per, h->rec_idx, h->rec_ret, h->rec_sign, h->rec_len, ordered);
    HCHECK(h, hipGetLastError());
    std::vector<PairRecord> host(n_global);
    HCHECK(h, hipMemcpyAsync(host.data(), ordered, (size_t)n_global * sizeof(PairRecord), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->rec_idx_host.resize(n_global);
    for (int i = 0; i < n_global; i++) h->rec_idx_host[i] = host[i].noise_idx;
    h->rec_n = n_global;
    if (records_out) memcpy(records_out, host.data(), (size_t)n_global * sizeof(PairRecord));
    return check_records_host(h, n_global);
}

// Test hook for the one piece of the N > 1 exchange that a one-GPU box cannot reach through RCCL: the device-side un-sharding
// of a [world][per] all-gather result into global pair order.  gathered: what ncclAllGather would have produced.
extern "C" int dne_debug_unshard(dne_handle *h, const void *gathered, int n_global, int world, void *ordered_out) {
    DeviceGuard dg(h);
    if (n_global < 1 || world < 1) return h->fail("dne_debug_unshard: bad sizes");
    const int per = (n_global + world - 1) / world;
    if (rec_reserve(h, n_global, per * world)) return -1;
    PairRecord *g = (PairRecord *)h->rec_recv, *ordered = g + (size_t)per * world;
    HCHECK(h, hipMemcpyAsync(g, gathered, (size_t)per * world * sizeof(PairRecord), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_records_unpack, dim3((n_global + 255) / 256), dim3(256), 0, h->stream, (const PairRecord *)g, n_global, world, per,
                       h->rec_idx, h->rec_ret, h->rec_sign, h->rec_len, ordered);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipMemcpyAsync(ordered_out, ordered, (size_t)n_global * sizeof(PairRecord), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// es.py:281-298 on the gathered, device-resident records: process returns, aggregate, optimizer step
extern "C" int dne_es_update_gathered(dne_handle *h, int proc_mode, int opt_kind, float l2, double stepsize, double b1m, double b2,
                                      double eps, double *ratio) {
    DeviceGuard dg(h);
    const int n = h->rec_n, n2 = 2 * n;
    if (n < 1) return h->fail("dne_es_update_gathered: no gathered records (dne_allgather_results / dne_records_set first)");
    float *proc = h->scratch_f, *w = h->scratch_f + n2;
    if (proc_mode == DNE_PROC_CENTERED_RANK) {          // es.py:281-282
        hipLaunchKernelGGL(k_centered_ranks, dim3((n2 + 255) / 256), dim3(256), 0, h->stream, (const float *)h->rec_ret, n2, proc);
    } else if (proc_mode == DNE_PROC_SIGN) {            // es.py:283-284
        HCHECK(h, hipMemcpyAsync(proc, h->rec_sign, n2 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    } else if (proc_mode == DNE_PROC_CENTERED_SIGN_RANK) {   // es.py:285-286
        hipLaunchKernelGGL(k_centered_ranks, dim3((n2 + 255) / 256), dim3(256), 0, h->stream, (const float *)h->rec_sign, n2, proc);
    } else {
        return h->fail("unknown return_proc_mode %d", proc_mode);
    }
    hipLaunchKernelGGL(k_pair_weights, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const float *)proc, n, w);
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    hipLaunchKernelGGL(k_weighted_sum, dim3((h->L.P + 255) / 256), dim3(256), 0, h->stream, (const float *)h->noise,
                       (const int64_t *)h->rec_idx, (const float *)w, n, h->L.P, (float)n2, h->g);   // es.py:296 g /= returns_n2.size
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    h->prof.reduce_ms = ms;
    return dne_optimizer_step(h, opt_kind, l2, stepsize, b1m, b2, eps, ratio);
}

extern "C" int dne_es_update(dne_handle *h, const int64_t *idx, const float *returns_n2, const float *signreturns_n2, int n,
                             int proc_mode, int opt_kind, float l2, double stepsize, double b1m, double b2, double eps,
                             double *ratio) {
    DeviceGuard dg(h);
    if (n < 1) return h->fail("dne_es_update: n = %d unsupported", n);
    if (proc_mode != DNE_PROC_CENTERED_RANK && !signreturns_n2) return h->fail("this return_proc_mode needs signreturns_n2");
    std::vector<PairRecord> rec(n);
    for (int i = 0; i < n; i++) {
        rec[i].noise_idx = idx[i];
        rec[i].ret[0] = returns_n2[2 * i]; rec[i].ret[1] = returns_n2[2 * i + 1];
        rec[i].len[0] = rec[i].len[1] = 0;
        rec[i].sign[0] = signreturns_n2 ? signreturns_n2[2 * i] : 0.0f; rec[i].sign[1] = signreturns_n2 ? signreturns_n2[2 * i + 1] : 0.0f;
    }
    if (dne_records_set(h, rec.data(), n)) return -1;
    return dne_es_update_gathered(h, proc_mode, opt_kind, l2, stepsize, b1m, b2, eps, ratio);
}

extern "C" int dne_ga_select(dne_handle *h, const float *returns, int m, int t, int32_t *out_idx) {
    DeviceGuard dg(h);
    if (m < 1 || t < 1 || t > m) return h->fail("dne_ga_select: bad sizes m = %d t = %d", m, t);
    if (rec_reserve(h, m, 1)) return -1;
    HCHECK(h, hipMemcpyAsync(h->scratch_f, returns, m * sizeof(float), hipMemcpyHostToDevice, h->stream));
    int32_t *out = (int32_t *)(h->scratch_f + m);
    hipLaunchKernelGGL(k_ga_select, dim3((m + 255) / 256), dim3(256), 0, h->stream, (const float *)h->scratch_f, m, t, out);
    HCHECK(h, hipMemcpyAsync(out_idx, out, t * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the novelty archive lives on the device: the master's archive only ever grows (nses.py:246-247 appends one BC per
// iteration), so a worker uploads each entry once instead of the whole archive on every call
static size_t row_pitch(int dim) { return ((size_t)dim + 15) & ~(size_t)15; }

// rows of `dim` bytes laid out at the device pitch (zero pad bytes add nothing to a squared difference)
static int upload_rows(dne_handle *h, uint8_t *dst, const uint8_t *src, size_t rows, int dim) {
    const size_t pitch = row_pitch(dim);
    if (pitch == (size_t)dim) return copy_h2d(h, dst, src, rows * dim);
    std::vector<uint8_t> pad(rows * pitch, 0);
    for (size_t r = 0; r < rows; r++) std::memcpy(pad.data() + r * pitch, src + r * dim, dim);
    return copy_h2d(h, dst, pad.data(), pad.size());
}

static int archive_reserve(dne_handle *h, size_t rows, size_t entries, int dim) {
    const size_t pitch = row_pitch(dim);
    if (rows * pitch > h->arch_cap) {
        uint8_t *nb = nullptr;
        const size_t cap = std::max<size_t>(2 * rows * pitch, 1u << 20);
        HCHECK(h, h->alloc(&nb, cap, "novelty_archive"));
        if (h->arch && h->arch_rows) HCHECK(h, hipMemcpy(nb, h->arch, h->arch_rows * h->arch_pitch, hipMemcpyDeviceToDevice));
        HCHECK(h, h->release(h->arch));
        h->arch = nb; h->arch_cap = cap;
    }
    if (entries > h->arch_ent_cap) {
        const size_t cap = std::max<size_t>(2 * entries, 256);
        HCHECK(h, h->release(h->arch_row0)); HCHECK(h, h->release(h->arch_len));
        HCHECK(h, h->alloc(&h->arch_row0, cap, "novelty_row0")); HCHECK(h, h->alloc(&h->arch_len, cap, "novelty_len"));
        h->arch_ent_cap = cap;
        if (!h->arch_len_host.empty()) {
            HCHECK(h, hipMemcpy(h->arch_row0, h->arch_row0_host.data(), h->arch_row0_host.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            HCHECK(h, hipMemcpy(h->arch_len, h->arch_len_host.data(), h->arch_len_host.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
    }
    return 0;
}

extern "C" int dne_archive_clear(dne_handle *h) {
    DeviceGuard dg(h);
    HCHECK(h, hipStreamSynchronize(h->stream));
    h->arch_rows = 0; h->arch_dim = 0; h->arch_pitch = 0;
    h->arch_row0_host.clear(); h->arch_len_host.clear();
    return 0;
}

extern "C" int dne_archive_append(dne_handle *h, const uint8_t *bc, int bc_len, int dim) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_archive_append");
    if (bc_len < 1 || dim < 1) return h->fail("dne_archive_append: empty entry");
    if (h->arch_dim && dim != h->arch_dim) return h->fail("dne_archive_append: entry width %d, archive holds %d", dim, h->arch_dim);
    HCHECK(h, hipStreamSynchronize(h->stream));
    const size_t n = h->arch_len_host.size();
    if (archive_reserve(h, h->arch_rows + bc_len, n + 1, dim)) return -1;
    h->arch_dim = dim; h->arch_pitch = row_pitch(dim);
    if (upload_rows(h, h->arch + h->arch_rows * h->arch_pitch, bc, bc_len, dim)) return -1;
    const int64_t row0 = (int64_t)h->arch_rows; const int32_t len = bc_len;
    HCHECK(h, hipMemcpy(h->arch_row0 + n, &row0, sizeof(row0), hipMemcpyHostToDevice));
    HCHECK(h, hipMemcpy(h->arch_len + n, &len, sizeof(len), hipMemcpyHostToDevice));
    h->arch_row0_host.push_back(row0); h->arch_len_host.push_back(len);
    h->arch_rows += bc_len;
    return 0;
}

extern "C" int dne_archive_size(dne_handle *h) { return (int)h->arch_len_host.size(); }

// a caller-supplied archive replaces the resident one (the one-shot form of the two novelty calls)
static int archive_load(dne_handle *h, const uint8_t *archive, const int32_t *alen, int narch, int dim) {
    if (narch < 1) return h->fail("empty archive");
    if (dne_archive_clear(h)) return -1;
    size_t rows = 0;
    for (int a = 0; a < narch; a++) { if (alen[a] < 1) return h->fail("empty archive entry"); rows += alen[a]; }
    if (archive_reserve(h, rows, narch, dim)) return -1;
    h->arch_dim = dim; h->arch_pitch = row_pitch(dim);
    if (upload_rows(h, h->arch, archive, rows, dim)) return -1;
    int64_t r0 = 0;
    for (int a = 0; a < narch; a++) { h->arch_row0_host.push_back(r0); h->arch_len_host.push_back(alen[a]); r0 += alen[a]; }
    HCHECK(h, hipMemcpy(h->arch_row0, h->arch_row0_host.data(), narch * sizeof(int64_t), hipMemcpyHostToDevice));
    HCHECK(h, hipMemcpy(h->arch_len, h->arch_len_host.data(), narch * sizeof(int32_t), hipMemcpyHostToDevice));
    h->arch_rows = rows;
    return 0;
}

template <typename T>
static int novelty_grow(dne_handle *h, T *&p, size_t &cap, size_t need, const char *name) {
    if (need <= cap) return 0;
    HCHECK(h, h->release(p));
    cap = std::max<size_t>(2 * need, 4096);
    HCHECK(h, h->alloc(&p, cap, name));
    return 0;
}

// nses.py:22-32 for n trajectories against the resident archive, whose width the caller has checked against `dim`:
// bcs == NULL scores the recorded trajectories (member i at row i * bc_max_steps), otherwise the host rows uploaded here.
// Both sides go to the kernels in length order (novelty.h); only the n results come back.
static int novelty_run(dne_handle *h, const uint8_t *bcs, const int32_t *lengths, int n, int k, double *out) {
    const int narch = (int)h->arch_len_host.size(), dim = h->arch_dim, pw = (int)(h->arch_pitch / 4);
    const uint32_t *mrows = (const uint32_t *)h->bc;
    std::vector<int64_t> mrow0(n);
    int64_t rows = 0;
    for (int i = 0; i < n; i++) { mrow0[i] = bcs ? rows : (int64_t)i * h->cfg.bc_max_steps; rows += lengths[i]; }
    if (bcs) {
        if (novelty_grow(h, h->nov_rows, h->nov_rows_cap, (size_t)rows * h->arch_pitch, "novelty_rows")) return -1;
        if (upload_rows(h, h->nov_rows, bcs, rows, dim)) return -1;
        mrows = (const uint32_t *)h->nov_rows;
    }
    std::vector<int32_t> mo(n), ao(narch);
    for (int i = 0; i < n; i++) mo[i] = i;
    for (int a = 0; a < narch; a++) ao[a] = a;
    std::stable_sort(mo.begin(), mo.end(), [&](int x, int y) { return lengths[x] < lengths[y]; });
    std::stable_sort(ao.begin(), ao.end(), [&](int x, int y) { return h->arch_len_host[x] < h->arch_len_host[y]; });
    // one upload: [member row0][archive row0] int64, then [member len][archive len][member order] int32
    std::vector<int64_t> r0((size_t)n + narch);
    std::vector<int32_t> ln(2 * (size_t)n + narch);
    for (int i = 0; i < n; i++) { r0[i] = mrow0[mo[i]]; ln[i] = lengths[mo[i]]; ln[(size_t)n + narch + i] = mo[i]; }
    for (int a = 0; a < narch; a++) { r0[(size_t)n + a] = h->arch_row0_host[ao[a]]; ln[(size_t)n + a] = h->arch_len_host[ao[a]]; }
    const size_t b64 = r0.size() * sizeof(int64_t), bytes = b64 + ln.size() * sizeof(int32_t);
    if (novelty_grow(h, h->nov_idx, h->nov_idx_cap, bytes, "novelty_index")) return -1;
    if (novelty_grow(h, h->nov_dist, h->nov_dist_cap, (size_t)n * narch + n, "novelty_dist")) return -1;
    HCHECK(h, hipMemcpyAsync(h->nov_idx, r0.data(), b64, hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->nov_idx + b64, ln.data(), bytes - b64, hipMemcpyHostToDevice, h->stream));
    const int64_t *d_r0 = (const int64_t *)h->nov_idx;
    const int32_t *d_ln = (const int32_t *)(h->nov_idx + b64);
    double *d_res = h->nov_dist + (size_t)n * narch;
    // fewer tiles than two per CU: split each tile's rows over more workgroups, up to one per staged step of the longest
    const int tx = (n + NV_T - 1) / NV_T, ty = (narch + NV_T - 1) / NV_T, tiles = tx * ty;
    const int maxlen = std::max(lengths[mo[n - 1]], h->arch_len_host[ao[narch - 1]]);
    const int steps = (int)(((int64_t)maxlen * ((pw + NV_W - 1) / NV_W) + NV_R - 1) / NV_R);
    const int rsplit = tiles >= 512 ? 1 : std::max(1, std::min((512 + tiles - 1) / tiles, steps));
    const size_t pairs = (size_t)n * narch;
    if (rsplit > 1) {
        if (novelty_grow(h, h->nov_acc, h->nov_acc_cap, 2 * pairs, "novelty_acc")) return -1;
        HCHECK(h, hipMemsetAsync(h->nov_acc, 0, 2 * pairs * sizeof(unsigned long long), h->stream));
    }
    hipLaunchKernelGGL(k_knn_dist, dim3(tx, ty, rsplit), dim3(256), 0, h->stream,
                       mrows, d_r0, d_ln, n, (const uint32_t *)h->arch, d_r0 + n, d_ln + n, narch, pw, h->nov_acc, h->nov_dist);
    HCHECK(h, hipGetLastError());
    if (rsplit > 1) {
        hipLaunchKernelGGL(k_knn_finish, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, h->stream,
                           (const unsigned long long *)h->nov_acc, pairs, h->nov_dist);
        HCHECK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_knn_select, dim3((n + 3) / 4), dim3(256), 0, h->stream, (const double *)h->nov_dist, n, narch,
                       std::min(k, narch), d_ln + n + narch, d_res);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipMemcpyAsync(out, d_res, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int dne_novelty_knn(dne_handle *h, const uint8_t *bcs, const int32_t *lengths, int n, int dim, int k, double *out) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_novelty_knn");
    if (n < 1 || dim < 1 || k < 1) return h->fail("dne_novelty_knn: bad sizes n = %d dim = %d k = %d", n, dim, k);
    if (!bcs) {
        if (!es_like(h->L.kind) || !h->bc || h->cfg.bc_final_only) return h->fail("dne_novelty_knn on the recorded trajectories needs an ES engine created with record_bc = 1 (full trajectories)");
        if (check_n(h, n)) return -1;
        if (dim != 128) return h->fail("dne_novelty_knn: the recorded trajectories are 128-byte RAM rows, not %d", dim);
    }
    const int narch = (int)h->arch_len_host.size();
    if (narch < 1) return h->fail("dne_novelty_knn: the archive is empty");
    if (dim != h->arch_dim) return h->fail("dne_novelty_knn: characterisation width %d, archive holds %d", dim, h->arch_dim);
    for (int i = 0; i < n; i++) {
        if (lengths[i] < 1 || (!bcs && lengths[i] > h->cfg.bc_max_steps))
            return h->fail("member %d: trajectory length %d outside [1, %d]", i, lengths[i], bcs ? INT_MAX : h->cfg.bc_max_steps);
    }
    return novelty_run(h, bcs, lengths, n, k, out);
}

// nses.py:12-32.  archive == NULL: score against the device-resident archive (dne_archive_append)
extern "C" int dne_novelty(dne_handle *h, const uint8_t *archive, const int32_t *alen, int narch, const uint8_t *bc,
                           int bc_len, int dim, int k, double *out) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_novelty");
    if (bc_len < 1 || dim < 1 || k < 1) return h->fail("dne_novelty: bad sizes");
    if (archive && archive_load(h, archive, alen, narch, dim)) return -1;
    narch = (int)h->arch_len_host.size();
    if (narch < 1) return h->fail("dne_novelty: the archive is empty");
    if (dim != h->arch_dim) return h->fail("dne_novelty: characterisation width %d, archive holds %d", dim, h->arch_dim);
    return novelty_run(h, bc, &bc_len, 1, k, out);
}

extern "C" int dne_novelty_batch(dne_handle *h, const uint8_t *archive, const int32_t *alen, int narch, int n,
                                 const int32_t *lengths, int k, double *out) {
    DeviceGuard dg(h);
    MAZE_REFUSE(h, "dne_novelty_batch");
    if (!es_like(h->L.kind) || !h->bc || h->cfg.bc_final_only) return h->fail("dne_novelty_batch needs an ES engine created with record_bc = 1 (full trajectories)");
    if (check_n(h, n)) return -1;
    if (k < 1) return h->fail("dne_novelty_batch: bad sizes");
    if (archive && archive_load(h, archive, alen, narch, 128)) return -1;
    narch = (int)h->arch_len_host.size();
    if (narch < 1) return h->fail("dne_novelty_batch: the archive is empty");
    if (h->arch_dim != 128) return h->fail("dne_novelty_batch: the archive must hold 128-byte RAM rows");
    for (int i = 0; i < n; i++)
        if (lengths[i] < 1 || lengths[i] > h->cfg.bc_max_steps) return h->fail("member %d: trajectory length %d outside the recorded capacity %d", i, lengths[i], h->cfg.bc_max_steps);
    return novelty_run(h, nullptr, lengths, n, k, out);
}

// ---- pool novelty over final RAM states (GA-NS on Atari; csrc/ram_novelty.h) ----------------------------------------
// what every call below needs of the resident archive: empty, or 128 bytes wide with every entry of length 1 (entry e is then row e)
static int ram_check_archive(dne_handle *h, const char *call) {
    const size_t A = h->arch_len_host.size();
    if (A && h->arch_dim != ram_novelty::ROW) return h->fail("%s: the archive holds entries of width %d, a RAM point has %d bytes", call, h->arch_dim, ram_novelty::ROW);
    for (size_t e = 0; e < A; e++)
        if (h->arch_len_host[e] != 1) return h->fail("%s: archive entry %zu has length %d, a RAM point is an entry of length 1", call, e, h->arch_len_host[e]);
    return 0;
}

// the engine keeps one final RAM row per member of its last evaluation in bc
static int ram_check_recorded(dne_handle *h, const char *call) {
    if (!h->bc) return h->fail("%s: the engine was created with record_bc = 0, it keeps no final RAM states", call);
    if (es_like(h->L.kind) && !h->cfg.bc_final_only)
        return h->fail("%s: the engine records full trajectories (an ES kind without bc_final_only), not one final RAM state per member", call);
    if (h->ram_last_n < 1) return h->fail("%s: no evaluation has left final RAM states yet", call);
    return 0;
}

// rows[i] = the bc row of the caller's member members[i] of the last evaluation (members == NULL: members 0 .. count - 1); identity reports
// whether that is rows[i] = i
static void ram_rows_of(dne_handle *h, const int32_t *members, int count, std::vector<int32_t> &rows, bool &identity) {
    std::vector<int32_t> inv(h->ram_last_n);
    for (int j = 0; j < h->ram_last_n; j++) inv[h->ram_last_caller[j]] = j;
    rows.resize(count);
    identity = true;
    for (int i = 0; i < count; i++) { rows[i] = inv[members ? members[i] : i]; identity = identity && rows[i] == i; }
}

extern "C" int dne_ram_novelty_pool(dne_handle *h, const uint8_t *bc, int n, int k, double *out, int32_t *neighbours) {
    DeviceGuard dg(h);
    const char *call = "dne_ram_novelty_pool";
    MAZE_REFUSE(h, call);
    if (n < 1) return h->fail("%s: n = %d, at least one member is needed", call, n);
    if (k < 1) return h->fail("%s: k = %d, at least one neighbour is needed", call, k);
    if (k > DNE_RAM_NOVELTY_KMAX) return h->fail("%s: k = %d, the kernel keeps at most DNE_RAM_NOVELTY_KMAX = %d neighbours", call, k, DNE_RAM_NOVELTY_KMAX);
    if (!out) return h->fail("%s: no output buffer", call);
    if (!bc) {
        if (ram_check_recorded(h, call)) return -1;
        if (n > h->ram_last_n) return h->fail("%s: %d members asked for, the last evaluation ran %d", call, n, h->ram_last_n);
    }
    if (ram_check_archive(h, call)) return -1;
    const size_t A = h->arch_len_host.size();
    if (A + (size_t)n - 1 < 1) return h->fail("%s: the pool is empty (one member, no archive point)", call);
    if (A + (size_t)n > (size_t)INT_MAX) return h->fail("%s: %zu combined slots would not fit the kernel's 31-bit slot field", call, A + (size_t)n);
    const int narch = (int)A, kk = (int)std::min<size_t>((size_t)k, A + (size_t)n - 1);
    const uint8_t *pts = nullptr;
    if (bc) {
        if (novelty_grow(h, h->ram_pts, h->ram_pts_cap, (size_t)n * ram_novelty::ROW, "ram_novelty_points")) return -1;
        if (copy_h2d(h, h->ram_pts, bc, (size_t)n * ram_novelty::ROW)) return -1;
        pts = h->ram_pts;
    } else {
        std::vector<int32_t> rows; bool identity;
        ram_rows_of(h, nullptr, n, rows, identity);
        pts = h->bc;
        if (!identity) {   // the evaluation reordered its members: the population in the caller's order, device to device
            if (novelty_grow(h, h->ram_pts, h->ram_pts_cap, (size_t)n * ram_novelty::ROW, "ram_novelty_points")) return -1;
            if (novelty_grow(h, h->ram_idx, h->ram_idx_cap, (size_t)n, "ram_novelty_rows")) return -1;
            HCHECK(h, hipMemcpyAsync(h->ram_idx, rows.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(ram_novelty::k_ram_archive_gather, dim3((unsigned)(((size_t)n * 8 + 255) / 256)), dim3(256), 0, h->stream,
                               (const uint32_t *)h->bc, (const int32_t *)h->ram_idx, n, (uint32_t *)h->ram_pts);
            HCHECK(h, hipGetLastError());
            HCHECK(h, hipStreamSynchronize(h->stream));   // rows goes away
            pts = h->ram_pts;
        }
    }
    if (novelty_grow(h, h->ram_out, h->ram_out_cap, (size_t)n, "ram_novelty_out")) return -1;
    if (neighbours && novelty_grow(h, h->ram_nb, h->ram_nb_cap, (size_t)n * kk, "ram_novelty_neighbours")) return -1;
    HCHECK(h, hipEventRecord(h->ev_a, h->stream));
    hipLaunchKernelGGL(ram_novelty::k_ram_novelty_pool, dim3((n + ram_novelty::MEMBERS - 1) / ram_novelty::MEMBERS), dim3(ram_novelty::THREADS), 0, h->stream,
                       (const uint32_t *)pts, n, (const uint32_t *)(narch ? h->arch : nullptr), narch, kk, h->ram_out, neighbours ? h->ram_nb : (int32_t *)nullptr);
    HCHECK(h, hipGetLastError());
    HCHECK(h, hipEventRecord(h->ev_b, h->stream));
    HCHECK(h, hipMemcpyAsync(out, h->ram_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (neighbours) HCHECK(h, hipMemcpyAsync(neighbours, h->ram_nb, (size_t)n * kk * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    HCHECK(h, hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
    h->ram_last_ms = ms;
    return 0;
}

// archive entry A + i = the final RAM of the last evaluation's member members[i] (the caller's indices), device to device; the indices are
// checked before anything is launched, and the gather follows archive_reserve's reallocation on the engine's stream
extern "C" int dne_archive_append_members(dne_handle *h, const int32_t *members, int count) {
    DeviceGuard dg(h);
    const char *call = "dne_archive_append_members";
    MAZE_REFUSE(h, call);
    if (count < 1) return h->fail("%s: count = %d, at least one member is needed", call, count);
    if (!members) return h->fail("%s: no member indices", call);
    if (ram_check_recorded(h, call)) return -1;
    for (int i = 0; i < count; i++)
        if (members[i] < 0 || members[i] >= h->ram_last_n)
            return h->fail("%s: index %d is member %d, the last evaluation ran %d", call, i, members[i], h->ram_last_n);
    if (h->arch_dim && h->arch_dim != ram_novelty::ROW) return h->fail("dne_archive_append: entry width %d, archive holds %d", ram_novelty::ROW, h->arch_dim);
    const size_t A = h->arch_len_host.size();
    if (A + (size_t)count > (size_t)INT_MAX) return h->fail("%s: %zu entries would not fit an int", call, A + (size_t)count);
    std::vector<int32_t> rows; bool identity;
    ram_rows_of(h, members, count, rows, identity);
    HCHECK(h, hipStreamSynchronize(h->stream));
    if (archive_reserve(h, h->arch_rows + count, A + count, ram_novelty::ROW)) return -1;
    if (novelty_grow(h, h->ram_idx, h->ram_idx_cap, (size_t)count, "ram_novelty_rows")) return -1;
    h->arch_dim = ram_novelty::ROW; h->arch_pitch = row_pitch(ram_novelty::ROW);
    HCHECK(h, hipMemcpyAsync(h->ram_idx, rows.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(ram_novelty::k_ram_archive_gather, dim3((unsigned)(((size_t)count * 8 + 255) / 256)), dim3(256), 0, h->stream,
                       (const uint32_t *)h->bc, (const int32_t *)h->ram_idx, count, (uint32_t *)(h->arch + h->arch_rows * h->arch_pitch));
    HCHECK(h, hipGetLastError());
    for (int i = 0; i < count; i++) { h->arch_row0_host.push_back((int64_t)h->arch_rows + i); h->arch_len_host.push_back(1); }
    HCHECK(h, hipMemcpyAsync(h->arch_row0 + A, h->arch_row0_host.data() + A, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipMemcpyAsync(h->arch_len + A, h->arch_len_host.data() + A, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HCHECK(h, hipStreamSynchronize(h->stream));   // rows and the caller's buffer are free again
    h->arch_rows += count;
    return 0;
}

extern "C" int dne_archive_get_points(dne_handle *h, int first, int count, uint8_t *out) {
    DeviceGuard dg(h);
    const char *call = "dne_archive_get_points";
    MAZE_REFUSE(h, call);
    const size_t A = h->arch_len_host.size();
    if (count < 1) return h->fail("%s: count = %d, at least one entry is needed", call, count);
    if (first < 0 || (size_t)first + (size_t)count > A) return h->fail("%s: entries %d .. %lld asked for, the archive holds %zu", call, first, (long long)first + count - 1, A);
    if (!out) return h->fail("%s: no buffer", call);
    if (h->arch_dim != ram_novelty::ROW) return h->fail("%s: the archive holds entries of width %d, a RAM point has %d bytes", call, h->arch_dim, ram_novelty::ROW);
    for (int e = first; e < first + count; e++)
        if (h->arch_len_host[e] != 1) return h->fail("%s: archive entry %d has length %d, a RAM point is an entry of length 1", call, e, h->arch_len_host[e]);
    HCHECK(h, hipStreamSynchronize(h->stream));
    return copy_d2h(h, out, h->arch + (size_t)h->arch_row0_host[first] * h->arch_pitch, (size_t)count * ram_novelty::ROW);
}

extern "C" double dne_ram_novelty_last_ms(dne_handle *h) { return h->episodic() ? -1.0 : h->ram_last_ms; }

// the same header on the CPU: no handle, no GPU
extern "C" int dne_ram_novelty_pool_host(const uint8_t *bc, int n, const uint8_t *archive, int narch, int k, double *out, int32_t *neighbours) {
    const char *call = "dne_ram_novelty_pool_host";
    if (!bc || !out || (narch > 0 && !archive)) { g_create_error = std::string(call) + ": a buffer is missing"; return -1; }
    if (n < 1) { g_create_error = std::string(call) + ": n = " + std::to_string(n) + ", at least one member is needed"; return -1; }
    if (narch < 0) { g_create_error = std::string(call) + ": narch = " + std::to_string(narch); return -1; }
    if (k < 1) { g_create_error = std::string(call) + ": k = " + std::to_string(k) + ", at least one neighbour is needed"; return -1; }
    if ((long long)narch + n - 1 < 1) { g_create_error = std::string(call) + ": the pool is empty (one member, no archive point)"; return -1; }
    if ((long long)narch + n > (long long)INT_MAX) { g_create_error = std::string(call) + ": " + std::to_string((long long)narch + n) + " combined slots would not fit the 31-bit slot field"; return -1; }
    ram_novelty::novelty_pool_host(bc, n, archive, narch, k, out, neighbours);
    return 0;
}
