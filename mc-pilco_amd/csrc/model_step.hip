// ONE differentiable time step of an mcp_model for gfx950 (MI355X), for closed loops whose policy the fused rollouts do not know: the caller
// evaluates its policy in torch and hands (x_t, u_t) to
//   mcp_model_step       x_{t+1}, optionally the GP means / variances and the record jac [M][G][D] = d delta_g / dz, one launch
//   mcp_model_step_bwd   (g_x, g_u) from g_{x_{t+1}} and the record, one launch
// Replaces Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718) inside the generic loops of
// MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674) and MC_PILCO4PMS.apply_policy (:808-906): the feature map in torch, one
// posterior launch per GP, Normal(...).rsample(), the integrator, and what autograd records of them.
//
// Within a step no GP waits for another, and every state component is integrated from exactly one GP's increment.  So the forward grid is
// (tiles of PT particles) x G: the workgroup of (tile, g) forms z for its particles, runs phases K, V, J, J' of rollout_open_phases.h for
// GP g alone -- the functions rollout_open.hip instantiates, on 512 threads dealt the same way, so a chain of steps carries the bits of
// mcp_rollout_open -- and in phase F writes the components that delta_g determines: x'[vel[g]] and, where not_vel[g] >= 0, x'[not_vel[g]].
// A component that no GP integrates is written as zero by the workgroups of GP 0 (mcp_rollout_open's value).  There is no hand-off between
// workgroups and no workspace.  noise->eps is THIS step's row [M][G]; without it Philox is addressed by the step index t.
//
// The reverse launch has no atomics and no sums across particles: stages A - C of rollout_open_bwd_kernel for one row.
#include "rollout_open_phases.h"

using namespace mcp;

struct StepArgs {
  OpenArgs o;  // the open-loop arguments of a two-row rollout: x0 = x, states = x_next, mu / var / jac [M][G](..), T = 2, no lengths
  int t;       // the step's index in its rollout (Philox addressing only)
};

struct StepLayout {
  int xs, z, red, gpl, kpar, panel, vpan, wj, redj, total;  // offsets in doubles
};
// (red keeps rollout_open.hip's [2][G][RF_NW][PT] indexing although a workgroup fills its own GP's slots only: open_wjs reads it that way)
__host__ __device__ inline StepLayout step_layout(int PT, bool needvar, bool needjac, int S, int D, int G, int NpadMax, int na) {
  StepLayout L;
  int o = 0;
  auto take = [&](int n) {
    int r = o;
    o += (n + 1) & ~1;
    return r;
  };
  L.xs = take(PT * S);
  L.z = take(PT * D);
  L.red = take(2 * G * RF_NW * PT);
  L.gpl = take(GPL_DOUBLES);
  L.kpar = take(KP_STRIDE(D));
  const int rj = needjac ? RF_NW * na * (D + 1) * PT : 0;  // phase J's partial sums [wave][column][D + 1][PT]: over the k panel, dead after V
  L.panel = needvar ? take(imax(NpadMax * RO_KR(PT), rj)) : 0;
  L.vpan = (needvar && needjac) ? take(NpadMax * RO_KR(PT)) : 0;
  L.wj = (needvar && needjac) ? take(PT) : 0;
  L.redj = needvar ? L.panel : (needjac ? take(rj) : 0);
  L.total = o;
  return L;
}

template <int PT, int MAXDEG, bool NEEDVAR, bool NEEDJAC>
__global__ __launch_bounds__(RF_NT) void model_step_kernel(StepArgs sa) {
  extern __shared__ double smem[];
  const OpenArgs& a = sa.o;
  const mcp_model& md = a.model;
  const int S = md.S, U = md.U, G = md.G, D = md.D, M = a.M;
  const int nna = md.n_not_angle, na = md.n_angle;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.y, m0 = blockIdx.x * PT;
  const StepLayout L = step_layout(PT, NEEDVAR, NEEDJAC, S, D, G, a.NpadMax, a.na);
  double* xs = smem + L.xs;
  double* z = smem + L.z;
  double* red = smem + L.red;
  GpL* gpl = reinterpret_cast<GpL*>(smem + L.gpl);
  double* kpar = smem + L.kpar;
  double* panel = smem + L.panel;
  double* vpan = smem + L.vpan;
  double* wjl = smem + L.wj;
  double* redj = smem + L.redj;
  const mcp_noise nzl = noise_of_launch(a.nz);
  const int tn = nzl.eps ? 0 : sa.t;  // the eps buffer is this step's row; Philox counts the step of the rollout

  stage_gp_tables(md.gp + g, md.var_scale + g, 1, D, gpl, kpar, tid);
  // ---- phase S: thread (p, s) owns state component s of particle p of the tile; the next PT * U threads fetch the inputs ----
  const bool own = tid < PT * S;
  const int op = own ? tid / S : 0, os = own ? tid - op * S : 0;
  const int ut = tid - PT * S;
  const bool isu = ut >= 0 && ut < PT * U;
  const int up = isu ? ut / U : 0, uk = isu ? ut - up * U : 0;
  const int tp = own ? op : up;
  const int om = imin(m0 + tp, M - 1);
  const bool ovalid = m0 + tp < M;
  unsigned bad = 0;
  int g_vel = -1, g_pos = -1;  // the GP this component is the velocity / the position of, as rollout_open_kernel finds them
  if (own) {
    const double xn = a.x0[(size_t)om * S + os];
    int zi_plain = -1, zi_ang = -1;
    for (int i = 0; i < nna; ++i)
      if (md.not_angle[i] == os) zi_plain = i;
    for (int i = 0; i < na; ++i)
      if (md.angle[i] == os) zi_ang = i;
    for (int h = 0; h < G; ++h) {
      if (md.vel[h] == os) g_vel = h;
      if (md.not_vel[h] == os) g_pos = h;
    }
    xs[op * S + os] = xn;
    if (ovalid && is_bad(xn)) bad |= MCP_STATUS_NAN;
    double* zp = z + op * D;
    if (zi_plain >= 0) zp[zi_plain] = xn;
    if (zi_ang >= 0) {
      double sn, cs;
      sincos_fast(xn, &sn, &cs);
      zp[nna + zi_ang] = sn;
      zp[nna + na + zi_ang] = cs;
    }
  }
  if (isu) {
    const double uv = a.u[(size_t)om * U + uk];
    z[up * D + nna + 2 * na + uk] = uv;
    if (ovalid && is_bad(uv)) bad |= MCP_STATUS_NAN;
  }
  __syncthreads();
  // ---- phases K, V, J, J' for GP g ----
  const GpL gp = gpl[0];
  open_phase_k<PT, MAXDEG, NEEDVAR>(gp, kpar, D, z, panel, red + g * RF_NW * PT, tid, wv, lane, gp.Xt, gp.alpha, gp.Npad);
  if (NEEDJAC && !NEEDVAR)  // the mean step: beta = alpha, nothing of phase K is needed
    open_phase_j<PT, MAXDEG, false>(gp, kpar, D, z, nullptr, 0.0, redj, a.na, wv, lane, gp.Xt, gp.alpha, gp.Npad);
  lds_barrier();
  if (NEEDVAR) {
    const int Npad = __builtin_amdgcn_readfirstlane(gp.Npad);
    double q = 0.0;
    for (int I0 = 32 * wv; I0 < Npad; I0 += 32 * RF_NW) q += open_v_block<PT, NEEDJAC>(gp.Kinv, Npad, I0, panel, vpan, lane);
    q = fold_kk(q);
    if (lane < PT) red[(G + g) * RF_NW * PT + wv * PT + lane] = q;
    lds_barrier();  // the panel is rewritten by phase J's partial sums
    if (NEEDJAC) {
      const int nn = (lane & 15) < PT ? (lane & 15) : 0;
      const double wjs = open_wjs<PT, MAXDEG>(a, nzl, gp, kpar, D, G, g, tn, imin(m0 + nn, M - 1), z + nn * D, red, nn);
      if (wv == 0 && lane < PT) wjl[lane] = wjs;
      open_phase_j<PT, MAXDEG, true>(gp, kpar, D, z, vpan, wjs, redj, a.na, wv, lane, gp.Xt, gp.alpha, gp.Npad);
      lds_barrier();
    }
  }
  if (NEEDJAC) open_jac_store<PT, MAXDEG, NEEDVAR>(a, gp, kpar, g, 0, m0, z, NEEDVAR ? wjl : nullptr, redj, a.na, tid);
  // ---- phase F: moments, sample, integrate   v' = v + delta ;  q' = q + Ts v + Ts/2 delta   (Model_learning.py:711-716) ----
  if (own && ovalid) {
    double* xo = a.states + (size_t)(m0 + op) * S;
    const bool isvel = g_vel == g, ispos = g_pos == g;  // (a position integrates its own GP's increment, as there)
    if (isvel || ispos) {
      const double* zp = z + op * D;
      double mu = gp.mean;
#pragma unroll
      for (int w = 0; w < RF_NW; ++w) mu += red[g * RF_NW * PT + w * PT + op];
      double var = 0.0, dv = mu;
      if (NEEDVAR) {
        double ktv = 0.0;
#pragma unroll
        for (int w = 0; w < RF_NW; ++w) ktv += red[(G + g) * RF_NW * PT + w * PT + op];
        double kzz = gp.lambda;
        if (MAXDEG >= 1 && gp.deg >= 1) {
          double p1 = kpar[KP_W1(D) + D];
          for (int d = 0; d < D; ++d) p1 = fma(kpar[KP_W1(D) + d] * zp[d], zp[d], p1);
          kzz += p1;
          if (MAXDEG >= 2 && gp.deg >= 2) {
            double Sa = 0.0, Sb = 0.0;
            for (int d = 0; d < D; ++d) {
              const double zz = zp[d] * zp[d];
              Sa = fma(kpar[KP_W20(D) + d], zz, Sa);
              Sb = fma(kpar[KP_W21(D) + d], zz, Sb);
            }
            kzz = fma(Sa, Sb, kzz);
          }
        }
        var = (kzz - ktv) * gp.var_scale;
        if (a.sample) {
          const double e = nzl.eps ? nzl.eps[((size_t)tn * M + om) * G + g] : philox_normal(nzl, om, tn, g);
          dv = fma(sqrt(var), e, mu);
        }
      }
      if (isvel) {  // every GP has exactly one velocity component: its thread reports
        const size_t o = (size_t)(m0 + op) * G + g;
        if (a.mu) a.mu[o] = mu;
        if (NEEDVAR && a.var) a.var[o] = var;
        if (a.sample && var <= 0.0) bad |= MCP_STATUS_NONPOS_VAR;  // (finite and not positive: a NaN variance is MCP_STATUS_NAN)
        if (is_bad(mu) || is_bad(var)) bad |= MCP_STATUS_NAN;
      }
      const double* xc = xs + op * S;
      const double nx = ispos ? xc[os] + md.Ts * xc[md.vel[g]] + 0.5 * md.Ts * dv : xc[os] + dv;
      if (ispos || g_pos < 0) {
        xo[os] = nx;
        if (is_bad(nx)) bad |= MCP_STATUS_NAN;
      }
    } else if (g == 0 && g_vel < 0 && g_pos < 0) {
      xo[os] = 0.0;
    }
  }
  if (bad) atomicOr(a.status, bad);
}

// ---------------------------------------------------------------------------------------
// The reverse step: what autograd's backward does through one get_next_state and the feature map, from the record alone -- one row of
// rollout_open_bwd_kernel (rollout_open.hip), the same order of operations, lam' = g_next:
//   A  gd_g    = sum over the components s that integrate GP g of  lam'[s]  (a velocity, a delta-state component) or  Ts/2 lam'[s]  (a position)
//   B  gz[d]   = sum_g gd_g jac[m][g][d]   in index order
//   C  g_x[s]  = lam'[s] (s is integrated at all) + Ts lam'[not_vel[g]] (s = vel[g] of a position) + gz through z = [x_not_angle, sin, cos, u]:
//                gz[i] | gz[sin_i] cos x - gz[cos_i] sin x;     g_u[k] = gz[nna + 2 na + k]
// A workgroup owns SB_PT particles; lane (particle, g / d / component) per stage, the stages meet in LDS.
// ---------------------------------------------------------------------------------------
#define SB_PT 16
#define SB_NT 128

struct StepBwdArgs {
  int S, U, G, D, nna, na, M;
  int angle[MCP_MAX_STATE], not_angle[MCP_MAX_STATE], vel[MCP_MAX_GP], not_vel[MCP_MAX_GP];
  double Ts;
  const double* x;
  const double* jac;
  const double* g_next;
  double* g_x;
  double* g_u;
};

__global__ __launch_bounds__(SB_NT) void model_step_bwd_kernel(StepBwdArgs a) {
  __shared__ double lam[SB_PT * MCP_MAX_STATE], gdl[SB_PT * MCP_MAX_GP], gzl[SB_PT * MCP_MAX_GPDIM];
  __shared__ int ogt[MCP_MAX_STATE], post[MCP_MAX_STATE], velof[MCP_MAX_STATE], zplain[MCP_MAX_STATE], zang[MCP_MAX_STATE];
  const int S = a.S, U = a.U, G = a.G, D = a.D, M = a.M, nna = a.nna, na = a.na;
  const int tid = threadIdx.x, m0 = blockIdx.x * SB_PT;
  if (tid < S) {  // which GP a component integrates, as the forward kernel decides it
    const int s = tid;
    int g_vel = -1, g_pos = -1, zp = -1, za = -1;
    for (int g = 0; g < G; ++g) {
      if (a.vel[g] == s) g_vel = g;
      if (a.not_vel[g] == s) g_pos = g;
    }
    for (int i = 0; i < nna; ++i)
      if (a.not_angle[i] == s) zp = i;
    for (int i = 0; i < na; ++i)
      if (a.angle[i] == s) za = i;
    ogt[s] = g_pos >= 0 ? g_pos : g_vel;
    post[s] = g_pos >= 0 ? 1 : 0;
    velof[s] = g_pos >= 0 ? a.vel[g_pos] : -1;
    zplain[s] = zp;
    zang[s] = za;
  }
  for (int it = tid; it < SB_PT * S; it += SB_NT) {
    const int p = it / S, s = it - p * S;
    lam[it] = m0 + p < M ? a.g_next[(size_t)(m0 + p) * S + s] : 0.0;
  }
  __syncthreads();
  for (int it = tid; it < SB_PT * G; it += SB_NT) {  // stage A
    const int p = it / G, g = it - p * G;
    double acc = 0.0;
    for (int s = 0; s < S; ++s)
      if (ogt[s] == g) acc += post[s] ? 0.5 * a.Ts * lam[p * S + s] : lam[p * S + s];
    gdl[it] = acc;
  }
  __syncthreads();
  for (int it = tid; it < SB_PT * D; it += SB_NT) {  // stage B
    const int p = it / D, d = it - p * D;
    double acc = 0.0;
    if (m0 + p < M) {
      const double* rc = a.jac + (size_t)(m0 + p) * G * D;
      for (int g = 0; g < G; ++g) acc = fma(gdl[p * G + g], rc[g * D + d], acc);
    }
    gzl[it] = acc;
  }
  __syncthreads();
  if (a.g_x) {
    for (int it = tid; it < SB_PT * S; it += SB_NT) {  // stage C
      const int p = it / S, s = it - p * S;
      if (m0 + p >= M) continue;
      const double* lamc = lam + p * S;
      double v = 0.0;
      if (ogt[s] >= 0) v += lamc[s];
      for (int s2 = 0; s2 < S; ++s2)
        if (velof[s2] == s) v = fma(a.Ts, lamc[s2], v);
      if (zplain[s] >= 0) v += gzl[p * D + zplain[s]];
      if (zang[s] >= 0) {
        double sn, cs;
        sincos_fast(a.x[(size_t)(m0 + p) * S + s], &sn, &cs);
        v += gzl[p * D + nna + zang[s]] * cs - gzl[p * D + nna + na + zang[s]] * sn;
      }
      a.g_x[(size_t)(m0 + p) * S + s] = v;
    }
  }
  if (a.g_u) {
    for (int it = tid; it < SB_PT * U; it += SB_NT) {
      const int p = it / U, k = it - p * U;
      if (m0 + p < M) a.g_u[(size_t)(m0 + p) * U + k] = gzl[p * D + nna + 2 * na + k];
    }
  }
}

// ---- host path: checks -> fill -> ladder (a refused call makes no HIP call) -------------------------------------------------------------
template <int PT, int MAXDEG, bool NEEDVAR, bool NEEDJAC>
static int launch_step(const StepArgs& sa, hipStream_t st) {
  const OpenArgs& a = sa.o;
  const StepLayout L = step_layout(PT, NEEDVAR, NEEDJAC, a.model.S, a.model.D, a.model.G, a.NpadMax, a.na);
  const size_t lds = (size_t)L.total * sizeof(double);
  if (lds > MCP_LDS_LIMIT) return MCP_ERR_LIMIT;
  MCP_ENSURE_MAX_LDS((model_step_kernel<PT, MAXDEG, NEEDVAR, NEEDJAC>));
  hipLaunchKernelGGL((model_step_kernel<PT, MAXDEG, NEEDVAR, NEEDJAC>), dim3((a.M + PT - 1) / PT, a.model.G), dim3(RF_NT), lds, st, sa);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
template <int PT, bool NEEDVAR, bool NEEDJAC>
static int launch_step_deg(const StepArgs& sa, int maxdeg, hipStream_t st) {
  return maxdeg == 0 ? launch_step<PT, 0, NEEDVAR, NEEDJAC>(sa, st) : launch_step<PT, 2, NEEDVAR, NEEDJAC>(sa, st);
}
// The ladder of tiles by LDS fit, as launch_open_tiles (rollout_open.hip).  With a variance 16 particles per workgroup, so that Kinv is
// streamed once for all of them, 4 where the panels of 16 do not fit (without a record that fits at every compiled limit at once:
// Npad = 4096 x 4 is 128 KB), and with the record's second panel one particle beyond Npad ~ 2450 (2 x 32 KB of panels at the limit).
template <bool NEEDJAC>
static int launch_step_tiles(const StepArgs& sa, int maxdeg, hipStream_t st) {
  int rc = launch_step_deg<16, true, NEEDJAC>(sa, maxdeg, st);
  if (rc == MCP_ERR_LIMIT) rc = launch_step_deg<4, true, NEEDJAC>(sa, maxdeg, st);
  if constexpr (NEEDJAC)
    if (rc == MCP_ERR_LIMIT) rc = launch_step_deg<1, true, true>(sa, maxdeg, st);
  return rc;
}

extern "C" int mcp_model_step(const mcp_model* model, const mcp_noise* noise, int M, int t, int particle_pred, const double* x, const double* u,
                              double* x_next, double* mean, double* var, double* jac, uint32_t* status, void* stream) {
  if (!model || !noise || !x || !u || !x_next || !status) return MCP_ERR_ARG;
  if (M <= 0 || t < 0) return MCP_ERR_ARG;
  if (!model_within_limits(model)) return MCP_ERR_LIMIT;
  if (!model_ok(model)) return MCP_ERR_ARG;
  StepArgs sa;
  const int maxdeg = open_fill(sa.o, model, noise, M, 2, particle_pred, x, u, M, nullptr, x_next, mean, var, jac, status);
  sa.t = t;
  hipStream_t st = (hipStream_t)stream;
  const bool needvar = sa.o.sample || var != nullptr;
  // the mean step touches no Kinv.  Without a record: one particle per workgroup.  With it: 4 -- phase K and phase J of 16 particles side by
  // side, with no barrier between them, do not fit the registers at degree 2, and 4 fit the LDS at every compiled limit (41 KB)
  if (!needvar) return jac ? launch_step_deg<4, false, true>(sa, maxdeg, st) : launch_step_deg<1, false, false>(sa, maxdeg, st);
  return jac ? launch_step_tiles<true>(sa, maxdeg, st) : launch_step_tiles<false>(sa, maxdeg, st);
}

// (runs from the record: the model's scalars and index lists are checked, model_lists_ok, and no GP descriptor is looked at)
extern "C" int mcp_model_step_bwd(const mcp_model* model, int M, const double* x, const double* jac, const double* g_next, double* g_x, double* g_u,
                                  void* stream) {
  if (!model || !x || !jac || !g_next) return MCP_ERR_ARG;
  if (M <= 0) return MCP_ERR_ARG;
  if (!model_within_limits(model, false)) return MCP_ERR_LIMIT;
  if (!model_lists_ok(model)) return MCP_ERR_ARG;
  if (!g_x && !g_u) return MCP_OK;  // nothing asked for
  StepBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.S = model->S, a.U = model->U, a.G = model->G, a.D = model->D, a.nna = model->n_not_angle, a.na = model->n_angle, a.M = M;
  for (int i = 0; i < MCP_MAX_STATE; ++i) a.angle[i] = model->angle[i], a.not_angle[i] = model->not_angle[i];
  for (int g = 0; g < MCP_MAX_GP; ++g) a.vel[g] = model->vel[g], a.not_vel[g] = model->not_vel[g];
  a.Ts = model->Ts;
  a.x = x;
  a.jac = jac;
  a.g_next = g_next;
  a.g_x = g_x;
  a.g_u = g_u;
  hipLaunchKernelGGL(model_step_bwd_kernel, dim3((M + SB_PT - 1) / SB_PT), dim3(SB_NT), 0, (hipStream_t)stream, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
