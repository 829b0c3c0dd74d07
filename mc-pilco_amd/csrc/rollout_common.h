// Shared by the rollout sources (rollout_fwd*.hip, rollout_bwd.hip, rollout_open.hip): feature maps of the dynamics model and of the
// policy, descriptor validation (model_within_limits, model_lists_ok, model_ok, meas_pairs_disjoint, meas_model_check, policy_ok).
#pragma once
#include <string.h>

#include "mcp_device.h"

#define MCP_LDS_LIMIT (160 * 1024)

// GP input z = [x[not_angle], sin x[angle], cos x[angle], u]   (Model_learning.py:670-683)
// policy feature s = [x_nonangle, COS, SIN] (Policy.py:326-333) or [x, x*_t - x] (:397-399)
__device__ __forceinline__ double policy_feature(const mcp_policy& pl, const double* x, int q, int t) {
  if (pl.kind == MCP_POLICY_ANGLES) {
    int nna = pl.n_non_angle, na = pl.n_angle;
    if (q < nna) return x[pl.non_angle[q]];
    if (q < nna + na) return cos(x[pl.angle[q - nna]]);
    return sin(x[pl.angle[q - nna - na]]);
  }
  if (pl.kind == MCP_POLICY_TRAJ) {
    if (q < pl.S) return x[q];
    return pl.target_traj[(size_t)t * pl.S + (q - pl.S)] - x[q - pl.S];
  }
  return x[q];
}

// hand-off buffer of the GP-sharded forward launch (rollout_fwd.hip): [clusters][2][G][P][2] granules of 8 bytes, clusters * P < M + 16 (a launch per chunk, each rounded up to whole clusters)
static inline size_t rollout_xch_bytes(int M, int G) { return ((size_t)(M + 16) * 2 * G * 2 * sizeof(unsigned long long) + 15) & ~(size_t)15; }
// partial policy sums of the GP-sharded 16-particle kernel: clusters x 2 (step parity) x members (<= G) x 16 particles x U x 2 granules
static inline size_t rollout_uxch_bytes(int M, int G, int U) { return ((size_t)(M + 16) * 2 * G * U * 2 * sizeof(unsigned long long) + 15) & ~(size_t)15; }

// Packed phase-J operands of the 16-particle kernel's wide classes (D + 1 > 16; rollout_fwd_tile.hip, tile_xj_pack_kernel): per GP two
// variants ([X^T; 1] and its columns scaled by alpha_j) x two row tiles x (NpadMax / 8) x 64 lanes x 2 doubles, placed behind the hand-off
// granules in the caller's workspace.  0 for narrow models.
static inline size_t rollout_xj_bytes(const mcp_model* m) {
  if (!m || m->D + 1 <= 16 || m->D + 1 > 32) return 0;
  int npad = 0;
  for (int g = 0; g < m->G; ++g) npad = m->gp[g].Npad > npad ? m->gp[g].Npad : npad;
  return (size_t)m->G * 2 * 2 * (size_t)((npad + 7) / 8) * 64 * 2 * sizeof(double);
}

// Kinv as MFMA operand tiles for the lean small-swarm kernel (rollout_fwd.hip, kt_pack_kernel): G x NpadMax^2 doubles behind the
// packed phase-J operands in the caller's workspace, rebuilt by every call.  0 for models that kernel does not take.
#define RL_MAXD_ 8
static inline size_t rollout_kt_bytes(const mcp_model* m) {
  if (!m || m->D > RL_MAXD_ || m->G < 2) return 0;
  int npad = 0;
  for (int g = 0; g < m->G; ++g) npad = m->gp[g].Npad > npad ? m->gp[g].Npad : npad;
  if (npad > 640) return 0;
  return sizeof(double) * ((size_t)m->G * npad * npad + 6 * 128);  // (+ one register buffer of slack: the last stream may be read past its end)
}

// partial phase-F sums of the row-split cluster (FwdArgs.rxch): clusters x 2 (step parity) x G x 2 senders x 16 particles x (D + 1) columns x 2 values x
// 2 granules, last in the caller's workspace; wide models on swarms that can be resident at two workgroups per (tile, GP) only
static inline size_t rollout_rxch_bytes(const mcp_model* m, int M) {
  if (!m || rollout_xj_bytes(m) == 0 || M > 1024) return 0;
  return (size_t)((M + 15) / 16) * 2 * (size_t)m->G * 2 * 16 * (size_t)(m->D + 1) * 4 * sizeof(unsigned long long);  // (two senders: gsh_rs = 3)
}

// ---- descriptor checks: one home each.  The order every entry point keeps: NULL pointers and sizes (MCP_ERR_ARG), model_within_limits
// (MCP_ERR_LIMIT), model_ok or model_lists_ok (MCP_ERR_ARG), then its own descriptors ----
// the compiled limits of the model's dimensions and, unless `train` is false, of the training-set sizes (the sweeps of rollout_open.hip run
// from the record and never read a GP descriptor)
static inline bool model_within_limits(const mcp_model* m, bool train = true) {
  if (m->S > MCP_MAX_STATE || m->U > MCP_MAX_INPUT || m->G > MCP_MAX_GP || m->D > MCP_MAX_GPDIM) return false;
  for (int g = 0; train && g < m->G; ++g)
    if (m->gp[g].N > MCP_MAX_TRAIN) return false;
  return true;
}

// the model's scalars and index lists: ranges, D = n_not_angle + 2 n_angle + U, every index inside the state, no index twice in a list, no component
// written by two GPs.  No GP operand is looked at.
static inline bool model_lists_ok(const mcp_model* m) {
  if (!m) return false;
  if (m->S <= 0 || m->S > MCP_MAX_STATE || m->U <= 0 || m->U > MCP_MAX_INPUT || m->G <= 0 || m->G > MCP_MAX_GP) return false;
  if (m->D <= 0 || m->D > MCP_MAX_GPDIM) return false;
  if (m->n_angle < 0 || m->n_not_angle < 0 || m->n_not_angle + 2 * m->n_angle + m->U != m->D) return false;
  for (int i = 0; i < m->n_angle; ++i)
    if (m->angle[i] < 0 || m->angle[i] >= m->S) return false;
  for (int i = 0; i < m->n_not_angle; ++i)
    if (m->not_angle[i] < 0 || m->not_angle[i] >= m->S) return false;
  // not_vel[g] == -1: GP g has no integrated position (delta-state model, x'[vel] = x[vel] + delta)
  for (int g = 0; g < m->G; ++g)
    if (m->vel[g] < 0 || m->vel[g] >= m->S || m->not_vel[g] < -1 || m->not_vel[g] >= m->S) return false;
  // No index twice within angle or within not_angle: the kernels find a component's place in z with a last-match loop, so the slot of an
  // earlier entry would never be written.  (The same index in angle AND in not_angle is allowed: both slots are written.)
  for (int i = 0; i < m->n_angle; ++i)
    for (int j = 0; j < i; ++j)
      if (m->angle[i] == m->angle[j]) return false;
  for (int i = 0; i < m->n_not_angle; ++i)
    for (int j = 0; j < i; ++j)
      if (m->not_angle[i] == m->not_angle[j]) return false;
  // Every component is written by at most one GP, as its velocity or as its position: the forward kernels let the thread of vel[g] report
  // GP g's mu / var, and the sweeps keep one pull per component.
  for (int g = 0; g < m->G; ++g)
    for (int h = 0; h < m->G; ++h) {
      if (h < g && (m->vel[g] == m->vel[h] || (m->not_vel[g] >= 0 && m->not_vel[g] == m->not_vel[h]))) return false;
      if (m->vel[g] == m->not_vel[h]) return false;
    }
  return true;
}

// model_lists_ok plus the operands of every GP
static inline bool model_ok(const mcp_model* m) {
  if (!model_lists_ok(m)) return false;
  for (int g = 0; g < m->G; ++g) {
    const mcp_gp& gp = m->gp[g];
    if (gp.kern.D != m->D || gp.N <= 0 || gp.Npad < gp.N || (gp.Npad % 16) != 0 || gp.N > MCP_MAX_TRAIN) return false;
    if (!gp.Xt || !gp.X || !gp.alpha || !gp.Kinv || !gp.kern.inv_ls) return false;
    if (gp.kern.poly_deg < 0 || gp.kern.poly_deg > 2) return false;
    if (gp.kern.poly_deg >= 1 && (!gp.kern.w1 || !gp.aX)) return false;
    if (gp.kern.poly_deg >= 2 && (!gp.kern.w20 || !gp.kern.w21)) return false;
  }
  return true;
}

// every state component in at most one measurement pair, as position or as velocity (indices in range and n <= MCP_MAX_STATE: the caller's)
static inline bool meas_pairs_disjoint(const mcp_meas* ms) {
  for (int i = 0; i < ms->n; ++i)
    for (int j = 0; j < ms->n; ++j)
      if ((i != j && (ms->pos[i] == ms->pos[j] || ms->vel[i] == ms->vel[j])) || ms->pos[i] == ms->vel[j]) return false;
  return true;
}

// the measurement model of a measured feedback form (mcp_rollout_pd_meas, mcp_rollout_mlp_meas) against the model (host fields only).
// Every component belongs to at most one pair, as position or as velocity: the forward kernels give a pair to the thread of its position,
// the sweeps keep one filter adjoint per position component
static inline int meas_model_check(const mcp_model* model, const mcp_meas* ms) {
  if (ms->n < 0 || 2 * ms->n > model->S || ms->n > MCP_MAX_STATE) return MCP_ERR_ARG;
  if (ms->n == 0) return MCP_OK;
  if (!ms->meas || !(fabs(ms->a0) > 0.0) || !(model->Ts > 0.0)) return MCP_ERR_ARG;  // (a NaN a0 or Ts is refused too)
  for (int i = 0; i < ms->n; ++i)
    if (ms->pos[i] < 0 || ms->pos[i] >= model->S || ms->vel[i] < 0 || ms->vel[i] >= model->S) return MCP_ERR_ARG;
  return meas_pairs_disjoint(ms) ? MCP_OK : MCP_ERR_ARG;
}
// whether a measured entry runs its measured kernels (ms NULL: a plain entry; n == 0: the plain kernels on the same arguments)
static inline bool meas_active(const mcp_meas* ms) { return ms && ms->n > 0; }

// The refusals of a closed-loop entry (PD law, tanh MLP; rollout and sweep), in the order they all keep -- every one before any HIP call:
// `ptrs` (the entry's required pointers, the model among them) and the sizes (MCP_ERR_ARG), the compiled limits (MCP_ERR_LIMIT), the model
// (MCP_ERR_ARG), the policy's descriptor by `policy_check()` (its limit code first, then MCP_ERR_ARG), the measurement (ms NULL: none).
// `sweep`: the sweeps run from the record -- no training-set limits, model_lists_ok in model_ok's place -- and afterwards return MCP_OK
// themselves where no gradient is asked for.
template <class PolicyCheck>
static inline int closed_loop_checks(bool ptrs, int M, int T, const mcp_model* model, const mcp_meas* ms, bool sweep, PolicyCheck policy_check) {
  if (!ptrs || M <= 0 || T < 1) return MCP_ERR_ARG;
  if (!model_within_limits(model, !sweep)) return MCP_ERR_LIMIT;
  if (!(sweep ? model_lists_ok(model) : model_ok(model))) return MCP_ERR_ARG;
  const int prc = policy_check();
  if (prc != MCP_OK) return prc;
  return ms ? meas_model_check(model, ms) : MCP_OK;
}

// the model's part of a sweep's arguments (OpenBwdArgs, MlpBwdArgs: separate types, the same leading fields S .. T, index lists, Ts)
template <class Args>
static inline void sweep_fill_model(Args& a, const mcp_model* model, int M, int T) {
  a.S = model->S, a.U = model->U, a.G = model->G, a.D = model->D, a.nna = model->n_not_angle, a.na = model->n_angle, a.M = M, a.T = T;
  for (int i = 0; i < MCP_MAX_STATE; ++i) a.angle[i] = model->angle[i], a.not_angle[i] = model->not_angle[i];
  for (int g = 0; g < MCP_MAX_GP; ++g) a.vel[g] = model->vel[g], a.not_vel[g] = model->not_vel[g];
  a.Ts = model->Ts;
}

// policy-only evaluation (T == 1, no dynamics model): a stub model with no GPs
static inline mcp_model policy_only_model(const mcp_policy* p) {
  mcp_model m;
  memset(&m, 0, sizeof(m));
  m.S = p->S;
  m.U = p->U;
  m.G = 0;
  m.D = p->U;  // z = [u]
  m.Ts = 0.0;
  return m;
}

// the sweeps of the wide policy classes (<24,6>, <32,8>: P > 16 or U > 4) exist for up to 512 threads, one per basis function: the forward refuses
// what the backward could not differentiate (MCP_ERR_LIMIT from both)
static inline bool policy_basis_ok(const mcp_policy* p) { return !((p->P > 16 || p->U > 4) && p->B > MCP_MAX_BASIS_WIDE); }

static inline bool policy_ok(const mcp_policy* p, int S, int U, int T) {
  if (!p || p->S != S || p->U != U) return false;
  if (p->B <= 0 || p->B > MCP_MAX_BASIS || p->P <= 0 || p->P > MCP_MAX_PFEAT) return false;
  if (!p->log_ls || !p->centers || !p->weight || !p->u_max) return false;
  if (!(p->p_drop >= 0.0 && p->p_drop < 1.0)) return false;
  if (p->meas.n < 0 || 2 * p->meas.n > S) return false;
  for (int i = 0; i < p->meas.n; ++i)
    if (p->meas.pos[i] < 0 || p->meas.pos[i] >= S || p->meas.vel[i] < 0 || p->meas.vel[i] >= S || p->meas.pos[i] == p->meas.vel[i]) return false;
  if (p->meas.n > 0 && !(p->meas.a0 != 0.0)) return false;
  if (p->kind == MCP_POLICY_PLAIN) return p->P == S;
  if (p->kind == MCP_POLICY_ANGLES) {
    if (p->n_non_angle + 2 * p->n_angle != p->P) return false;
    for (int i = 0; i < p->n_angle; ++i)
      if (p->angle[i] < 0 || p->angle[i] >= S) return false;
    for (int i = 0; i < p->n_non_angle; ++i)
      if (p->non_angle[i] < 0 || p->non_angle[i] >= S) return false;
    return true;
  }
  if (p->kind == MCP_POLICY_TRAJ) return p->P == 2 * S && p->target_traj && p->traj_len >= T;
  return false;
}
