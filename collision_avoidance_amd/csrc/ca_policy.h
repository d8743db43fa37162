// ca_policy.h -- the kernels of a closed-loop policy rollout (ca_policy_actions, ca_rollout_policy)
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
//
// A policy is a ReLU MLP over an agent's 64-float observation with one output, the heading offset ca_step takes (include/ca_env.h
// ca_policy_desc).  Its definition is a k-ordered chain of fused multiply-adds that starts from the bias,
//     acc = b[j];  for k ascending: acc = fmaf(x[k], W[j][k], acc)
// which is what v_mfma_f32_16x16x4_f32 computes with the bias in C and successive instructions taking ascending k: the products of
// one instruction are added in the order k = 0 .. 3 of its lane groups.  policy_kernel<HEADS> runs on it, one kernel template with
// two output stages (policy_kernel<false>: the mean alone; policy_kernel<true>: the heads of a PPO sample, below):
//   * one wave per workgroup owns POLICY_ROWS = 32 rows (agents): two 16-row tiles, i.e. two independent accumulators per output tile,
//     which covers the instruction's dependent latency, and every weight fragment loaded serves both;
//   * the rows' observations are staged into LDS with 128-bit loads (and go to the obs record from the same registers); a layer reads
//     its A operand from LDS -- lane l holds x[row l & 15][4 s + (l >> 4)] of k-step s -- and writes its activations back to a second
//     LDS image in [row][column] order, so the next layer again walks k in ascending order: nothing is ever permuted along k;
//   * the weights come from global memory in the order the B operand wants them (the host packs them: [16-column tile][k-step][lane],
//     lane l holding W[16 jt + (l & 15)][4 s + (l >> 4)]), one coalesced 256-byte load per instruction; the output layer is a tile whose
//     column 0 -- lanes 0, 16, 32, 48 -- holds the rows' means, and whose columns 1 .. 15 are zero (with heads: 3 .. 15);
//   * an LDS row is width + 4 floats long: the A reads of a k-step and the D writes of a tile then touch 64 different banks.
// A row's result depends on its own observation and its arena's weight set only: not on the tiling, not on the rows beside it.
// policy_record_kernel is the accumulate kernel of a policy rollout: the rule of actseq_account (ca_actseq.h) with the reward and done
// records.
#pragma once
#include "ca_common.h"
#include "ca_actseq.h"

namespace ca {

enum { POLICY_ROWS = 32, POLICY_MAX_LAYERS = 4, POLICY_PAD = 4 };

struct PolicyArgs {
    const float* obs;           // [A*N][64], 16-byte aligned
    const float* wp;            // packed weights: [P][wset]
    const float* bp;            // biases: [P][bset]
    const int* set_of_arena;    // [A], or null: set 0 for every arena
    const float* noise;         // [A*N], or null
    float* actions;             // [A*N]
    float* actions_rec;         // [A*N] the action record's row, or null
    float* obs_rec;             // [A*N][64] the observation record's row, or null
    unsigned wp_off[POLICY_MAX_LAYERS], bp_off[POLICY_MAX_LAYERS];   // a layer's place inside a set
    unsigned wset, bset;        // floats per set
    unsigned an;                // A * N
    int N;
    int tpa;                    // tiles per arena (a tile holds rows of one arena), or 0: tiles of consecutive rows across arenas
    int n_layers;
    int width[POLICY_MAX_LAYERS + 1];
    int stride;                 // floats per LDS row: the largest width + POLICY_PAD
    int clip;                   // CA_POLICY_OUT_CLIP
    float limit;
};

typedef float policy_f32x4 __attribute__((ext_vector_type(4)));

// ---- the heads of a PPO sample (ca_policy_set_heads, ca_policy_evaluate, ca_rollout_policy_sample; include/ca_env.h) ----------------
// The output tile of a policy with heads holds the mean row in column 0, the log-std row in column 1 and the value row in column 2:
// three chains for the MFMAs that computed one.  policy_kernel<true> is the kernel on that tile: everything up to the last layer's
// accumulators is policy_kernel<false>'s, and the output stage is its own: lanes col = 0, 1, 2 of every 16-lane group hold the three
// results of the same four rows (twice: two row tiles), so they go through the LDS image the last layer leaves free, as [column][row],
// and lane r < 32 picks up row r: one row per lane for the fp64 exponential, consecutive lanes on consecutive banks and consecutive
// addresses of every record.
struct ActorCriticArgs {
    PolicyArgs p;               // as policy_kernel<false> takes it; wp / bp: the sets with the heads' output tile; actions may be null here
    float* logp;                // [A*N], or null
    float* value;               // [A*N], or null
    float* mean;                // [A*N], or null
    float* log_std;             // [A*N], or null
    int has_logstd;             // a log-std head is installed (else ls = 0, std = 1)
    int values_only;            // the bootstrap row: the value column alone
};

template <bool HEADS> struct PolicyKernelArgs { typedef PolicyArgs type; };
template <> struct PolicyKernelArgs<true> { typedef ActorCriticArgs type; };
__device__ __forceinline__ const PolicyArgs& policy_part(const PolicyArgs& q) { return q; }
__device__ __forceinline__ const PolicyArgs& policy_part(const ActorCriticArgs& q) { return q.p; }

template <bool HEADS>
__global__ __launch_bounds__(64) void policy_kernel(const typename PolicyKernelArgs<HEADS>::type q) {
    extern __shared__ __attribute__((aligned(16))) float policy_lds[];   // [2][POLICY_ROWS][stride]
    const PolicyArgs& p = policy_part(q);
    const int lane = (int)threadIdx.x;
    unsigned g0;
    int nvalid, set = 0;
    if (p.tpa > 0) {
        const unsigned arena = blockIdx.x / (unsigned)p.tpa;
        const int i0 = (int)(blockIdx.x - arena * (unsigned)p.tpa) * POLICY_ROWS;
        g0 = arena * (unsigned)p.N + (unsigned)i0;
        nvalid = p.N - i0 < POLICY_ROWS ? p.N - i0 : POLICY_ROWS;
        if (p.set_of_arena != nullptr) set = p.set_of_arena[arena];
    } else {
        g0 = blockIdx.x * (unsigned)POLICY_ROWS;
        nvalid = p.an - g0 < (unsigned)POLICY_ROWS ? (int)(p.an - g0) : POLICY_ROWS;
    }
    const int stride = p.stride;
    float* in = policy_lds;
    float* out = policy_lds + POLICY_ROWS * stride;
    // the tile's observations: 32 rows x 16 float4, eight per lane; rows past the end are zeros nobody reads back
#pragma unroll
    for (int it = 0; it < POLICY_ROWS * 16 / 64; ++it) {
        const int f4 = it * 64 + lane, row = f4 >> 4, c = (f4 & 15) * 4;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row < nvalid) {
            const size_t at = (size_t)(g0 + (unsigned)row) * CA_OBS_DIM + (size_t)c;
            v = *(const float4*)(p.obs + at);
            if (p.obs_rec != nullptr) *(float4*)(p.obs_rec + at) = v;
        }
        *(float4*)(in + row * stride + c) = v;
    }
    __syncthreads();
    const float* wset = p.wp + (size_t)set * p.wset;
    const float* bset = p.bp + (size_t)set * p.bset;
    const int col = lane & 15, grp = lane >> 4;
    for (int l = 0; l < p.n_layers; ++l) {
        const bool last = l == p.n_layers - 1;
        const int K = p.width[l], tiles = last ? 1 : p.width[l + 1] >> 4;
        const float* W = wset + p.wp_off[l];
        const float* B = bset + p.bp_off[l];
        const float* a0p = in + col * stride + grp;
        const float* a1p = a0p + 16 * stride;
        for (int jt = 0; jt < tiles; ++jt) {
            const float bias = B[jt * 16 + col];
            policy_f32x4 acc0 = {bias, bias, bias, bias}, acc1 = {bias, bias, bias, bias};
            const float* wj = W + (size_t)jt * (size_t)K * 16 + lane;
            for (int s0 = 0; s0 < (K >> 2); s0 += 4) {   // (K is a multiple of 16: four k-steps at a time, their loads in front)
                float b[4], x0[4], x1[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    b[u] = wj[(s0 + u) * 64];
                    x0[u] = a0p[(s0 + u) * 4];
                    x1[u] = a1p[(s0 + u) * 4];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[u], b[u], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[u], b[u], acc1, 0, 0, 0);
                }
            }
            if (!last) {   // D: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = grp * 4 + r;
                    out[row * stride + jt * 16 + col] = acc0[r] > 0.0f ? acc0[r] : 0.0f;
                    out[(row + 16) * stride + jt * 16 + col] = acc1[r] > 0.0f ? acc1[r] : 0.0f;
                }
            } else if constexpr (HEADS) {
                if (col < 3) {   // -> [column][row] in the free image, 3 x 32 floats
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        out[col * POLICY_ROWS + grp * 4 + r] = acc0[r];
                        out[col * POLICY_ROWS + grp * 4 + r + 16] = acc1[r];
                    }
                }
            } else if (col == 0) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int row = grp * 4 + (r & 3) + (r >> 2) * 16;
                    if (row < nvalid) {
                        const unsigned g = g0 + (unsigned)row;
                        float v = r < 4 ? acc0[r & 3] : acc1[r & 3];
                        if (p.noise != nullptr) v = __fadd_rn(v, p.noise[g]);
                        if (p.clip) v = fminf(fmaxf(v, -p.limit), p.limit);
                        p.actions[g] = v;
                        if (p.actions_rec != nullptr) p.actions_rec[g] = v;
                    }
                }
            }
        }
        __syncthreads();
        if (!HEADS || !last) { float* t = in; in = out; out = t; }   // (the heads' three columns stay in `out` for the epilogue)
    }
    if constexpr (HEADS) {   // one row per lane: value; sample, log-probability and the row's records
        if (lane >= nvalid) return;   // (nvalid <= 32: one row per lane)
        const unsigned g = g0 + (unsigned)lane;
        const float value = out[2 * POLICY_ROWS + lane];
        if (q.value != nullptr) q.value[g] = value;
        if (q.values_only) return;
        const float mean = out[lane], ls_raw = out[POLICY_ROWS + lane];
        float ls = 0.0f, sd = 1.0f;
        if (q.has_logstd) {
            ls = fminf(fmaxf(ls_raw, CA_POLICY_LOGSTD_MIN), CA_POLICY_LOGSTD_MAX);
            sd = (float)exp64((double)ls);
        }
        const float eps = p.noise != nullptr ? p.noise[g] : 0.0f;
        float u = __fadd_rn(mean, __fmul_rn(sd, eps));
        if (p.clip) u = fminf(fmaxf(u, -p.limit), p.limit);
        if (p.actions != nullptr) p.actions[g] = u;
        if (p.actions_rec != nullptr) p.actions_rec[g] = u;
        if (q.logp != nullptr) q.logp[g] = __fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(eps, eps)), ls), 0.918938533f);
        if (q.mean != nullptr) q.mean[g] = mean;
        if (q.log_std != nullptr) q.log_std[g] = ls;
    }
}
template __global__ void policy_kernel<false>(const PolicyArgs);
template __global__ void policy_kernel<true>(const ActorCriticArgs);

struct PolicyRecArgs {
    const float* reward;
    const int* arena_done;
    const int* entry_frozen;
    const int* agent_counts;   // [A] (ca_set_agent_counts), or null
    const float* weight;       // &weights[t], or null
    float* returns;            // or null
    int* first_done;
    float* rewards_rec;        // [A*N] row t of the reward record, or null
    int* done_rec;             // [A] row t of the done record, or null
    unsigned an;
    int A, N;
    int t;
    int freeze;
};

// behind the launches of step t: the step's records and the rule of the return and first_done (actseq_account, ca_actseq.h)
__global__ __launch_bounds__(256) void policy_record_kernel(const PolicyRecArgs s) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= s.an) return;
    const int a = (int)(g / (unsigned)s.N), i = (int)(g - (unsigned)a * (unsigned)s.N);
    actseq_account(g, a, i, s.reward[g], s.agent_counts, s.N, s.arena_done, s.entry_frozen, s.weight, s.returns, s.first_done, s.rewards_rec, s.done_rec, s.t,
                   s.freeze);
}

struct SampleRecArgs {
    PolicyRecArgs s;            // as policy_record_kernel takes it
    float* row_rewards;         // [A*N] row t / hold of the row-reward record, or null
    int* row_done;              // [A] row t / hold, or null
    int* row_valid;             // [A] row t / hold, or null
    int first;                  // t is the first step of its row
};

// behind the launches of step t of a sampling rollout: actseq_account as ever, then the row's records.  Whether the step advanced the
// arena is the rule of actseq_account read from the same words: first_done[a] is -1 or t in this launch where it was -1 before, and
// either says "advanced".
__global__ __launch_bounds__(256) void sample_record_kernel(const SampleRecArgs c) {
    const PolicyRecArgs& s = c.s;
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= s.an) return;
    const int a = (int)(g / (unsigned)s.N), i = (int)(g - (unsigned)a * (unsigned)s.N);
    const float r = s.reward[g];
    const int fd = s.first_done[a];
    const int done = s.arena_done[a];
    const int frozen0 = s.freeze ? s.entry_frozen[a] : 0;
    const float sum = c.row_rewards != nullptr && !c.first ? c.row_rewards[g] : 0.0f;
    const int rd = c.row_done != nullptr && !c.first && i == 0 ? c.row_done[a] : 0;
    const bool advanced = !(s.freeze && (frozen0 != 0 || (fd >= 0 && fd < s.t)));
    actseq_account(g, a, i, r, s.agent_counts, s.N, s.arena_done, s.entry_frozen, s.weight, s.returns, s.first_done, s.rewards_rec, s.done_rec, s.t,
                   s.freeze);
    if (c.row_rewards != nullptr && (c.first || advanced)) c.row_rewards[g] = advanced ? __fadd_rn(sum, r) : sum;
    if (i == 0) {
        if (c.row_done != nullptr) c.row_done[a] = rd | (done != 0 ? 1 : 0);
        if (c.row_valid != nullptr && c.first) c.row_valid[a] = advanced ? 1 : 0;
    }
}

struct GaeArgs {
    const float* rewards;       // [R][A*N]
    const float* values;        // [R+1][A*N]
    const int* done;            // [R][A]
    const int* valid;           // [R][A], or null: 1 everywhere
    float* adv;                 // [R][A*N], or null
    float* target;              // [R][A*N], or null
    unsigned an;
    int A, N, R;
    float gamma, gl;            // gl = gamma * lambda, one fp32 multiply on the host
};

enum { GAE_AHEAD = 4 };

// generalised advantage estimation (ca_gae; include/ca_env.h has the definition): one lane per agent, r = R-1 .. 0; the loads of
// GAE_AHEAD rows are issued in front of the chain that depends on the row above
__global__ __launch_bounds__(256) void gae_kernel(const GaeArgs s) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= s.an) return;
    const int a = (int)(g / (unsigned)s.N);
    const size_t an = s.an;
    float next_v = s.values[(size_t)s.R * an + g], next_a = 0.0f;
    for (int r0 = s.R - 1; r0 >= 0; r0 -= GAE_AHEAD) {
        float rew[GAE_AHEAD], val[GAE_AHEAD];
        int dn[GAE_AHEAD], vl[GAE_AHEAD];
#pragma unroll
        for (int u = 0; u < GAE_AHEAD; ++u) {
            const int r = r0 - u;
            const bool in = r >= 0;
            rew[u] = in ? s.rewards[(size_t)r * an + g] : 0.0f;
            val[u] = in ? s.values[(size_t)r * an + g] : 0.0f;
            dn[u] = in ? s.done[(size_t)r * s.A + a] : 0;
            vl[u] = in && s.valid != nullptr ? s.valid[(size_t)r * s.A + a] : 1;
        }
#pragma unroll
        for (int u = 0; u < GAE_AHEAD; ++u) {
            const int r = r0 - u;
            if (r < 0) break;
            const bool nd = dn[u] == 0;
            const float nv = nd ? next_v : 0.0f;
            const float delta = __fsub_rn(__fadd_rn(rew[u], __fmul_rn(s.gamma, nv)), val[u]);
            const float na = nd && r < s.R - 1 ? next_a : 0.0f;
            float adv = __fadd_rn(delta, __fmul_rn(s.gl, na));
            if (vl[u] == 0) adv = 0.0f;
            if (s.adv != nullptr) s.adv[(size_t)r * an + g] = adv;
            if (s.target != nullptr) s.target[(size_t)r * an + g] = __fadd_rn(adv, val[u]);
            next_v = val[u];
            next_a = adv;
        }
    }
}

}  // namespace ca
