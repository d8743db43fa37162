// ca_actseq.h -- the small kernels of an action-sequence rollout (ca_rollout_actions)
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
//
// The call is `steps` ca_step calls under the caller's [R, A, N] action tensor, row t / hold driving step t, plus two results of
// the caller's: returns [A, N], the weighted sum of the rewards of the steps that advanced the agent's arena, and first_done [A], the
// first step of the call that left arena_done set.  Two ways lead there:
//   * a handle whose step is a launch (or a launch sequence) of its own -- the one-lane kernels, the two-lanes kernel, the tiled path --:
//     every step is that launch with the step's row, and actseq_accumulate_kernel below runs behind it: the stream orders it behind the
//     reward and the arena_done the step stored; actseq_begin_kernel runs once in front and notes which arenas are frozen at entry;
//   * a handle whose rollout is one launch per 256 steps: the ActionSeq instantiations of the four-lanes kernel accumulate in a
//     register (ca_quad.h); actseq_setup_kernel writes their block into the handle's ActSeqDev in front of every such launch.
// The rule of the sum, in one place for both: ret = ret + w * r in two fp32 operations (ret + r where no weights were given).
#pragma once
#include "ca_common.h"

namespace ca {

// one step of the return: two roundings, never one (the library is built without contraction; the intrinsics say so here)
__device__ __forceinline__ float actseq_add(float ret, float w, float r) { return __fadd_rn(ret, __fmul_rn(w, r)); }

struct ActSeqBeginArgs {
    const int* arena_done;
    float* returns;       // or null
    int* first_done;      // the caller's, or the handle's own
    int* entry_frozen;    // [A], or null (the one-launch form has no use for it)
    unsigned an;
    int A;
    int freeze;           // CA_F_FREEZE is among the call's flags
};

// in front of the first step: returns = +0, first_done = -1, entry_frozen = the arena never advances in this call
__global__ __launch_bounds__(256) void actseq_begin_kernel(const ActSeqBeginArgs s) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (s.returns != nullptr && g < s.an) s.returns[g] = 0.0f;
    if (g < (unsigned)s.A) {
        s.first_done[g] = -1;
        if (s.entry_frozen != nullptr) s.entry_frozen[g] = (s.freeze && s.arena_done[g] != 0) ? 1 : 0;
    }
}

struct ActSeqAccArgs {
    const float* reward;
    const int* arena_done;
    const int* entry_frozen;
    const int* agent_counts;   // [A] (ca_set_agent_counts), or null
    const float* weight;       // &weights[t], or null
    float* returns;            // or null
    int* first_done;
    unsigned an;
    int A, N;
    int t;                     // the step of the call the launches in front of this one made
    int freeze;
};

// The accounting behind step t of a sequence call, for lane g = agent i of arena a whose reward of the step is r: the one statement of
// the rule for actseq_accumulate_kernel, policy_record_kernel (ca_policy.h) and nav_reward_kernel (ca_nav.h), each of which hands over
// the members of its argument block by value.  agent_counts / n_rows: the arena holds agent_counts[a] agents, n_rows where the pointer
// is null (a caller that has the count already passes it as n_rows); rewards_rec / done_rec: row t of a policy rollout's records, or
// null.  Under CA_F_FREEZE the step advanced arena a unless it was frozen at entry or an earlier step of the call left its flag set
// (first_done[a] in 0 .. t - 1).  The lane of agent 0 stores first_done[a] = t in this very launch at most; a lane of the same arena
// that reads it sees -1 or t, and decides the same either way.
__device__ __forceinline__ void actseq_account(unsigned g, int a, int i, float r, const int* agent_counts, int n_rows, const int* arena_done,
                                               const int* entry_frozen, const float* weight, float* returns, int* first_done,
                                               float* rewards_rec, int* done_rec, int t, int freeze) {
    // (every load is issued before anything is decided: the kernel is one memory latency long, not a chain of them)
    const float ret = returns != nullptr ? returns[g] : 0.0f;
    const int fd = first_done[a];
    const int done = arena_done[a];
    const int frozen0 = freeze ? entry_frozen[a] : 0;
    const int count = agent_counts != nullptr ? agent_counts[a] : n_rows;
    const float w = weight != nullptr ? *weight : 1.0f;
    if (rewards_rec != nullptr) rewards_rec[g] = r;   // (the records of every row and arena, frozen or not)
    if (done_rec != nullptr && i == 0) done_rec[a] = done;
    const bool advanced = !(freeze && (frozen0 != 0 || (fd >= 0 && fd < t)));
    if (!advanced) return;
    if (returns != nullptr && i < count) { float* const dst = returns + g; *dst = actseq_add(ret, w, r); }   // (the address first: the kernels' instruction order of before)
    if (i == 0 && fd < 0 && done != 0) first_done[a] = t;
}

// behind the launches of step t, one lane per agent, agent fastest
__global__ __launch_bounds__(256) void actseq_accumulate_kernel(const ActSeqAccArgs s) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= s.an) return;
    const int a = (int)(g / (unsigned)s.N), i = (int)(g - (unsigned)a * (unsigned)s.N);
    actseq_account(g, a, i, s.reward[g], s.agent_counts, s.N, s.arena_done, s.entry_frozen, s.weight, s.returns, s.first_done, nullptr, nullptr, s.t, s.freeze);
}

// the block of the next ActionSeq launch of the four-lanes kernel, by value through the kernel arguments: ordered on the stream like
// the launch that reads it, and no host memory has to outlive the call
__global__ void actseq_setup_kernel(ActSeqDev* dst, const ActSeqDev v) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst = v;
}

}  // namespace ca
