// The launch plans of mcp_rollout_fwd / mcp_rollout_bwd: which kernel family takes a call, at which width, with which parts of the
// workspace -- decided here, on the host, from the descriptors' scalars alone (no HIP call, no pointer inside a descriptor is followed), and
// then run by rollout_fwd.hip / rollout_bwd.hip.  mcp_rollout_fwd_plan / mcp_rollout_bwd_plan (include/mcpilco_hip_debug.h) return the same
// plans without a device.  DESIGN.md "Dispatch" has the order in which the families are tried.
#pragma once
#include "rollout_common.h"
#include "../../include/mcpilco_hip_debug.h"

#define RF_CW 128  // rows of v per column chunk of the small-tile kernels' Kinv stream: 64 lanes x 2 rows (one 16-byte load per lane)
#define RF_MAX_CHUNKS (MCP_MAX_GP * (MCP_MAX_TRAIN / 128))
#define BL_MAX_M 3072  // largest swarm the lean sweep takes (tools/sweep_bwd_particles.py on a 256-CU device: it wins up to ~3000 particles)
// the automatic row split of the GP-sharded 16-particle kernel: parts and deal
#define MCP_ROW_PARTS_DEFAULT 3
#define MCP_ROW_PART_MAJOR_DEFAULT 1
// a swarm goes out GP-sharded on the small-tile kernels when it fits this many resident grids (cart-pole shape, forward ms,
// tools/sweep_fwd_swarm.py: M=1024 two launches 4.9 vs 6.5 unsharded; M=1280 three launches 7.3 vs 6.9 on the tile kernel)
#define MCP_GP_MAX_LAUNCHES 2

namespace mcp {

// ---- host predicates of the kernels (defined beside the kernels whose LDS layouts they read) --------------------------------------------
// rollout_fwd.hip: dynamic LDS of the small-tile kernel at P particles per workgroup, GB GPs per pass; `sharded`: one GP per workgroup
size_t fwd_small_lds_bytes(const mcp_model* m, const mcp_policy* p, int P, int NpadMax, int maxdeg, int GB, int NCmax, bool xlds, bool sharded);
// rollout_fwd_tile.hip: the 16-particle kernel takes the shape; its GP-sharded launch does (classes 0 and 1, NpadMax <= 512)
bool fwd_tile_fits(const mcp_model* model, const mcp_policy* policy);
bool fwd_tile_sharded_takes(const mcp_model* model, const mcp_policy* policy, int NpadMax);
// rollout_fwd_lean.hip: dynamic LDS of the lean GP-sharded kernel at P particles per workgroup (0: it does not take the shape)
size_t fwd_lean_lds_bytes(const mcp_model* model, const mcp_policy* policy, int P, int NpadMax, int maxdeg);
// rollout_bwd.hip: the lean sweep covers the shape; the general sweep <PFM, ., MAXNT, ., PB> can launch NT threads for it (thread bounds,
// the prefetched record against BW_RPT, the LDS of bwd_layout)
bool bwd_lean_applies(const mcp_model* md, const mcp_policy* pl, int T);
bool bwd_sweep_fits(const mcp_model* md, const mcp_policy* pl, int PFM, int MAXNT, int PB, int NT);

// ---- the workspace of mcp_rollout_fwd: the one place that orders its regions --------------------------------------------------------------
//   xch   hand-off granules of the GP-sharded launches          (rollout_xch_bytes)
//   xj    packed phase-J operands of the wide 16-particle classes (rollout_xj_bytes; 0 for narrow models)
//   kt    Kinv as MFMA operand tiles of the lean kernel          (rollout_kt_bytes; 0 for models it does not take)
//   uxch  partial policy sums of the policy-split tile launch    (rollout_uxch_bytes)
//   rxch  partial phase-F sums of the row-split tile launch      (rollout_rxch_bytes; 0 beyond 1024 particles and for narrow models)
struct FwdWorkspace {
  size_t xch, xj, kt, uxch, rxch, total;  // byte offsets of the regions; a region ends where the next begins (rxch at `total`)
};
static inline FwdWorkspace fwd_workspace(const mcp_model* m, int M) {
  FwdWorkspace w;
  w.xch = 0;
  w.xj = w.xch + rollout_xch_bytes(M, m->G);
  w.kt = w.xj + rollout_xj_bytes(m);
  w.uxch = w.kt + rollout_kt_bytes(m);
  w.rxch = w.uxch + rollout_uxch_bytes(M, m->G, m->U);
  w.total = w.rxch + rollout_rxch_bytes(m, M);
  return w;
}
// a region is usable when it is not empty and the caller's buffer reaches its end
static inline bool ws_has(bool have, size_t bytes, size_t begin, size_t end) { return have && end > begin && bytes >= end; }

// ---- forward plan -------------------------------------------------------------------------------------------------------------------------
typedef mcp_fwd_plan FwdPlan;
typedef mcp_bwd_plan BwdPlan;

static inline int pick_particles_per_wg(int M) {
  // small swarms: spread over as many CUs as possible (every workgroup re-streams Kinv, so the
  // per-CU L2->L1 rate is the bound); large swarms: amortise the Kinv stream over more particles
  if (M <= 256) return 1;
  if (M <= 1024) return 2;
  return 16;  // falls back to 4 when the model does not fit the tile kernel
}

static inline int chunks_in_pass(const mcp_model* m, int GB) {
  int best = 0;
  for (int g0 = 0; g0 < m->G; g0 += GB) {
    int nc = 0;
    for (int g = g0; g < m->G && g < g0 + GB; ++g) nc += (m->gp[g].Npad + RF_CW - 1) / RF_CW;
    best = imax(best, nc);
  }
  return best;
}

// Workgroups per tile with which the GP-sharded 16-particle kernel can take the whole swarm in one resident grid (0 = it cannot): the largest
// divisor of G that fits, i.e. the fewest GPs per workgroup.  Every workgroup of a GP-sharded grid waits for its partners, so the whole grid
// must be resident: one 512-thread workgroup per CU (the LDS footprint allows no more).
static inline int tile_sharded_cluster(const mcp_model* m, const mcp_policy* p, int NpadMax, int M, int T, int cus) {
  if (m->G < 2 || T <= 1 || !fwd_tile_sharded_takes(m, p, NpadMax)) return 0;
  const int ncl = (M + 15) / 16;
  for (int cs = m->G; cs >= 2; --cs)
    if (m->G % cs == 0 && ((ncl + 7) / 8) * 8 * cs <= cus) return cs;
  return 0;
}

// what a forward call is given beside the descriptors
struct FwdCall {
  int M, T, flags;  // flags: the particle_pred argument (bit 0 and the MCP_FWD_* bits)
  bool have_workspace;
  size_t workspace_bytes;
  int cus;  // compute units of the device (0: unknown -- nothing is launched GP-sharded)
};

static inline int32_t ws_i32(size_t v) { return v > 0x7fffffffu ? 0x7fffffff : (int32_t)v; }
static inline void fwd_report_workspace(const FwdWorkspace& w, FwdPlan* pl) {
  pl->ws_xch = ws_i32(w.xch);
  pl->ws_xj = ws_i32(w.xj);
  pl->ws_kt = ws_i32(w.kt);
  pl->ws_uxch = ws_i32(w.uxch);
  pl->ws_rxch = ws_i32(w.rxch);
  pl->ws_total = ws_i32(w.total);
}
static inline void fwd_report(FwdPlan* pl) {
  const bool sharded = pl->family == MCP_FWD_SMALL_SHARDED || pl->family == MCP_FWD_LEAN || pl->family == MCP_FWD_TILE_SHARDED;
  pl->ran_particles = pl->particles;
  pl->ran_gp_sharded = sharded ? pl->launches : 0;
  pl->ran_fwd_lean = pl->family == MCP_FWD_LEAN;
  pl->ran_row_split = pl->gsh_rs > 1 ? pl->gsh_rs : 0;
}

// small swarms: the GPs of a particle cluster sharded over G workgroups (each streams one Kinv) when the whole grid is resident at one
// workgroup per CU; smallest cluster size first (most CUs busy); up to MCP_GP_MAX_LAUNCHES resident grids back to back
static inline bool plan_fwd_small_sharded(const mcp_model* m, const mcp_policy* p, const FwdCall& c, const mcp_dispatch* rq, bool kt_ok, bool tile_sh, FwdPlan* pl) {
  const int fp = rq->fwd_particles;
  const bool forced = fp == 1 || fp == 2 || fp == 4;
  int NC1 = 0;
  for (int g = 0; g < m->G; ++g) NC1 = imax(NC1, (m->gp[g].Npad + RF_CW - 1) / RF_CW);
  for (int P = forced ? fp : 1; P <= (forced ? fp : 4) && NC1 <= RF_MAX_CHUNKS; P <<= 1) {
    const int cap = (c.cus / (8 * m->G)) * 8 * P;  // particles one resident grid takes at this cluster size
    if (cap <= 0) break;
    const int nchunk = (c.M + cap - 1) / cap;
    if (nchunk > 1 && (P < 4 || nchunk > MCP_GP_MAX_LAUNCHES || (!forced && tile_sh))) continue;  // (the sharded 16-particle kernel is the faster form then)
    size_t lds = fwd_small_lds_bytes(m, p, P, pl->npad_max, pl->maxdeg, 1, NC1, true, true);
    bool lean = false;
    if (rq->fwd_lean != 1 && kt_ok) {
      const size_t ll = fwd_lean_lds_bytes(m, p, P, pl->npad_max, pl->maxdeg);
      if (ll > 0 && ll <= MCP_LDS_LIMIT) {
        lean = true;
        lds = ll;
      }
    }
    if (lds > MCP_LDS_LIMIT) break;
    pl->family = lean ? MCP_FWD_LEAN : MCP_FWD_SMALL_SHARDED;
    pl->particles = P;
    pl->xlds = 1;
    pl->gb = 1;
    pl->ncmax = NC1;
    pl->lds_bytes = (int32_t)lds;
    pl->launches = nchunk;
    pl->particles_per_launch = (((c.M + nchunk - 1) / nchunk + P - 1) / P) * P;  // whole clusters
    pl->zero_xch = 1;
    pl->pack_kt = lean && !(c.flags & MCP_FWD_KT_PACKED);  // (unless an earlier call left the tiles in the workspace)
    return true;
  }
  return false;
}

// swarms beyond one resident grid of the small-tile kernel, up to 2048 particles at two GPs: the 16-particle kernel GP-sharded, `cs` workgroups
// per tile; the policy split over them, and two or three workgroups per (tile, GP range) on row parts of Kinv, where the shape and the grid allow
static inline void plan_fwd_tile_sharded(const mcp_model* m, const mcp_policy* p, const FwdCall& c, const mcp_dispatch* rq, const FwdWorkspace& w, int cs,
                                         FwdPlan* pl) {
  const int ncl = (c.M + 15) / 16;
  pl->family = MCP_FWD_TILE_SHARDED;
  pl->particles = 16;
  pl->launches = 1;
  pl->particles_per_launch = c.M;
  pl->gsh_cs = cs;
  pl->zero_xch = 1;
  // the policy split (every member needs a tile of 16 basis functions).  Automatic: clusters of three or more on small swarms (the UR5 launch
  // script's M = 200: six members, the policy 1/6 of the step).  Not with two members -- the exchange costs what half a cart-pole policy does --
  // and not on large swarms, whose halves run another cluster size: they would no longer reproduce the whole bit for bit
  const bool want_split = rq->policy_split == 2 || (rq->policy_split != 1 && cs >= 3 && c.M <= 512);
  if (want_split && (p->B + 15) / 16 >= cs && ws_has(c.have_workspace, c.workspace_bytes, w.uxch, w.rxch)) pl->policy_split = pl->zero_uxch = 1;
  // the row split: wide classes with the per-tile phase J only (degree <= 1), three parts where three times the grid is resident, else two;
  // dealt row part major by default (one workgroup per CU, at most 32 per XCD)
  const bool can = pl->use_xj && pl->maxdeg <= 1 && pl->npad_max >= 128 && ws_has(c.have_workspace, c.workspace_bytes, w.rxch, w.total);
  const int map = rq->cluster_map == 1 ? 0 : (rq->cluster_map == 2 ? 1 : MCP_ROW_PART_MAJOR_DEFAULT);
  auto resident = [&](int rs) {
    return map == 1 ? ((ncl * cs * rs + 7) / 8) * 8 <= c.cus : ((ncl + 7) / 8) * 8 * cs * rs <= c.cus && ((ncl + 7) / 8) * cs * rs <= c.cus / 8;
  };
  if (can && rq->row_split != 1) {
    const int want = (rq->row_split == 2 || rq->row_split == 3) ? rq->row_split : MCP_ROW_PARTS_DEFAULT;
    const int rs = (want >= 3 && resident(3)) ? 3 : (resident(2) ? 2 : 1);
    if (rs > 1) {
      pl->gsh_rs = rs;
      pl->gsh_map = map;
      pl->zero_rxch = 1;
    }
  }
  pl->pack_xj = pl->use_xj && !(c.flags & MCP_FWD_XJ_PACKED);
}

// one workgroup per P particles, all GPs: most particles per workgroup first, operands in LDS if they fit, all GPs per pass if they fit
static inline bool plan_fwd_small(const mcp_model* m, const mcp_policy* p, const mcp_dispatch* rq, int P0, FwdPlan* pl) {
  for (int P = P0; P >= 1; P >>= 1)
    for (int xl = rq->fwd_no_xlds ? 0 : 1; xl >= 0; --xl)
      for (int GB = imax(1, rq->fwd_gb > 0 ? imin(rq->fwd_gb, m->G) : m->G); GB >= 1; --GB) {
        const int NCmax = chunks_in_pass(m, GB);
        if (NCmax > RF_MAX_CHUNKS) continue;
        const size_t lds = fwd_small_lds_bytes(m, p, P, pl->npad_max, pl->maxdeg, GB, NCmax, xl != 0, false);
        if (lds > MCP_LDS_LIMIT) continue;
        pl->family = MCP_FWD_SMALL;
        pl->particles = P;
        pl->xlds = xl;
        pl->gb = GB;
        pl->ncmax = NCmax;
        pl->lds_bytes = (int32_t)lds;
        pl->launches = 1;
        return true;
      }
  return false;
}

// The whole configuration search of mcp_rollout_fwd.  `model` may be NULL (policy-only evaluation, T == 1); `rq` is never NULL (a zeroed
// request is the automatic dispatch).  Returns MCP_OK with *pl filled, or the error the call returns with no family and no report words in *pl.
static inline int plan_fwd(const mcp_model* model, const mcp_policy* policy, const FwdCall& c, const mcp_dispatch* rq, FwdPlan* pl) {
  memset(pl, 0, sizeof(*pl));
  if (!policy || c.M <= 0 || c.T <= 0) return MCP_ERR_ARG;
  if (model && model->G >= 0 && model->G <= MCP_MAX_GP) fwd_report_workspace(fwd_workspace(model, c.M), pl);  // (the map needs no valid model)
  mcp_model stub;
  if (!model) {
    if (c.T != 1) return MCP_ERR_ARG;  // without a dynamics model only the policy can be evaluated
    stub = policy_only_model(policy);
    model = &stub;
  } else if (!model_ok(model)) {
    return MCP_ERR_ARG;
  }
  if (!policy_ok(policy, model->S, model->U, c.T)) return MCP_ERR_ARG;
  if (!policy_basis_ok(policy)) return MCP_ERR_LIMIT;
  int P0 = rq->fwd_particles ? rq->fwd_particles : pick_particles_per_wg(c.M);
  if (P0 != 1 && P0 != 2 && P0 != 4 && P0 != 16) return MCP_ERR_ARG;
  if (policy->meas.n > 0 && !policy->meas.meas) return MCP_ERR_ARG;
  for (int g = 0; g < model->G; ++g) {
    pl->npad_max = imax(pl->npad_max, model->gp[g].Npad);
    pl->maxdeg = imax(pl->maxdeg, model->gp[g].kern.poly_deg);
  }
  const FwdWorkspace w = fwd_workspace(model, c.M);
  pl->use_xj = ws_has(c.have_workspace, c.workspace_bytes, w.xj, w.kt);
  pl->use_kt = ws_has(c.have_workspace, c.workspace_bytes, w.kt, w.uxch);
  // GP-sharded forms: not when the request or the call's flag (the recovery path after MCP_STATUS_SYNC) says never, and only with the granules
  const bool may_shard = rq->gp_sharding != 1 && !(c.flags & MCP_FWD_NO_GP_SHARDING) && ws_has(c.have_workspace, c.workspace_bytes, w.xch, w.xj);
  const int tile_cs = may_shard ? tile_sharded_cluster(model, policy, pl->npad_max, c.M, c.T, c.cus) : 0;
  const int fp = rq->fwd_particles;
  bool done = false;
  if (may_shard && model->G >= 2 && c.T > 1 && (fp == 0 || (rq->gp_sharding == 2 && fp != 16)))
    done = plan_fwd_small_sharded(model, policy, c, rq, pl->use_kt != 0, tile_cs > 0, pl);
  if (!done && tile_cs > 0 && (P0 == 16 || fp == 0)) {
    plan_fwd_tile_sharded(model, policy, c, rq, w, tile_cs, pl);
    done = true;
  }
  if (!done && P0 == 16) {
    // large swarms: 16-particle tiles on the matrix cores (rollout_fwd_tile.hip) when the problem fits that kernel, else four per workgroup
    if (model->G >= 1 && c.T > 1 && fwd_tile_fits(model, policy)) {
      pl->family = MCP_FWD_TILE;
      pl->particles = 16;
      pl->launches = 1;
      pl->particles_per_launch = c.M;
      pl->pack_xj = pl->use_xj && !(c.flags & MCP_FWD_XJ_PACKED);
      done = true;
    }
    P0 = 4;
  }
  if (!done && !plan_fwd_small(model, policy, rq, P0, pl)) return MCP_ERR_LIMIT;  // (no family, no report words)
  if (pl->family == MCP_FWD_SMALL) pl->particles_per_launch = c.M;
  fwd_report(pl);
  return MCP_OK;
}

// ---- backward plan ------------------------------------------------------------------------------------------------------------------------
static inline int bwd_threads(int B) { return imax(64, ((B + 63) / 64) * 64); }
static inline int bwd_blocks(int M) { return imin(M, 1024); }
static inline size_t bwd_nparam_slab(const mcp_policy* p) { return (size_t)p->P + (size_t)p->B * p->P + (size_t)p->U * p->B + (size_t)p->U; }  // (+ U: dJ/dbias)

// bytes of the one workspace that serves both calls: the backward's per-workgroup gradient slabs or the forward's regions, whichever is larger
static inline size_t rollout_workspace_bytes(const mcp_model* model, const mcp_policy* policy, int M) {
  const size_t bwd = sizeof(double) * bwd_nparam_slab(policy) * (size_t)bwd_blocks(M);
  const size_t fwd = model ? fwd_workspace(model, M).total : 0;
  return bwd > fwd ? bwd : fwd;
}

// the instantiations of rollout_bwd_kernel that exist: sweep class <PFM, UM> x thread class MAXNT x particles per workgroup
static inline bool bwd_sweep_exists(int PFM, int MAXNT, int PB) {
  if (MAXNT == 256) return PB == 1 || PB == 2 || (PB == 4 && PFM == 8);
  if (MAXNT == 1024) return PB == 1;                                               // <8,2>, <16,4> beyond 256 basis functions
  return PB == 1 || PB == 2 || (PFM == 24 && (PB == 4 || PB == 8));                // 512: <24,6>, <32,8>
}

// The whole configuration search of mcp_rollout_bwd (as plan_fwd: `model` may be NULL, `rq` never).
static inline int plan_bwd(const mcp_model* model, const mcp_policy* policy, int M, int T, bool have_workspace, size_t workspace_bytes,
                           const mcp_dispatch* rq, BwdPlan* pl) {
  memset(pl, 0, sizeof(*pl));
  if (!have_workspace || !policy || M <= 0 || T <= 0) return MCP_ERR_ARG;
  if (policy->meas.n > 0 && !policy->meas.meas) return MCP_ERR_ARG;
  const bool with_model = model != nullptr;
  mcp_model stub;
  if (!model) {
    if (T != 1) return MCP_ERR_ARG;
    stub = policy_only_model(policy);
    model = &stub;
  } else if (!model_ok(model)) {
    return MCP_ERR_ARG;
  }
  if (!policy_ok(policy, model->S, model->U, T)) return MCP_ERR_ARG;
  if (!policy_basis_ok(policy)) return MCP_ERR_LIMIT;
  if (workspace_bytes < rollout_workspace_bytes(with_model ? model : nullptr, policy, M)) return MCP_ERR_WORKSPACE;
  const int PF = policy->P, U = policy->U, forced = rq->bwd_particles;
  // particles per workgroup: large swarms are latency bound per workgroup, so several particles share one sweep; small swarms keep one
  // particle per workgroup to spread over the CUs (two 256-thread workgroups per CU are resident: one particle per workgroup while M of
  // them fit in one round, then 2, then 4; tools/sweep_bwd_particles.py: M=800 1.74 / 1.34 / 1.92 ms, M=2000 3.24 / 2.51 / 2.07 ms for 1 / 2 / 4;
  // 2 particles win up to ~2800)
  int PB = forced ? forced : (M > 2816 ? 4 : (M > 512 ? 2 : 1));
  if (!forced && (PF > 16 || U > 4)) {
    // wide policies (tools/time_bwd.py, UR5 shape, M = 2000, T = 300: 18.1 / 15.5 / 14.5 ms for 1 / 2 / 4): four on large swarms, and eight
    // where that saves resident rounds -- a 512-thread workgroup of this class has a CU to itself (256 per round), and a step of eight particles
    // costs 1.86 x a step of four (tools/phase_stamps.py c5: 64.7 k vs 34.7 k cycles -- the RBF stage is per particle) -- M = 2000: one round
    // instead of two, 8.74 -> 8.1 ms; M = 3072: two instead of three, slower (16.8 vs 13.6 ms)
    PB = M > 1024 ? 4 : 1;
    const int r4 = (((M + 3) / 4) + 255) / 256, r8 = (((M + 7) / 8) + 255) / 256;
    if (PB == 4 && bwd_threads(policy->B) > 256 && 1.86 * r8 < (double)r4) PB = 8;  // (the 512-thread instantiation: > 256 basis functions)
  }
  if (PB != 1 && PB != 2 && PB != 4 && PB != 8) return MCP_ERR_ARG;
  if (rq->bwd_lean != 1 && !forced && M <= BL_MAX_M && with_model && bwd_lean_applies(model, policy, T)) {
    // small swarm, narrow class: the latency-lean sweep (wave 0 = the chain, the basis functions in the waves behind it), two particle slots
    // per workgroup, one launch per 512 particles = 256 workgroups: a resident round each
    pl->lean = pl->ran_bwd_lean = 1;
    pl->pfm = 8;
    pl->um = 2;
    pl->particles = 2;
    pl->threads = 2 * (64 + bwd_threads(policy->B));
    pl->launches = (M + 511) / 512;
    pl->slabs = imin(M, 1024);  // one per particle, modulo the 1024 the workspace holds
    return MCP_OK;
  }
  // the general sweep: the class follows from the policy's widths, the thread class from the thread count; a width that does not exist or does
  // not fit is halved
  pl->pfm = (PF <= 8 && U <= 2) ? 8 : ((PF <= 16 && U <= 4) ? 16 : ((PF <= 24 && U <= 6) ? 24 : MCP_MAX_PFEAT));
  pl->um = pl->pfm == 8 ? 2 : (pl->pfm == 16 ? 4 : (pl->pfm == 24 ? 6 : MCP_MAX_INPUT));
  for (; PB >= 1; PB >>= 1) {
    const int NT = imax(bwd_threads(policy->B), 64 * PB);
    // one particle per workgroup on the 512-thread wide instantiations, no measurement model, a wave to spare: the pipelined form (PIPEC)
    const int pipe = (PB == 1 && rq->bwd_pipe != 1 && pl->pfm > 16 && NT > 256 && NT + 64 <= 512 && policy->meas.n == 0) ? 1 : 0;
    const int maxnt = NT <= 256 ? 256 : (pl->pfm <= 16 ? 1024 : 512);
    if (!bwd_sweep_exists(pl->pfm, maxnt, PB) || !bwd_sweep_fits(model, policy, pl->pfm, maxnt, PB, NT + 64 * pipe)) continue;
    pl->maxnt = maxnt;
    pl->particles = PB;
    pl->threads = NT + 64 * pipe;
    pl->pipe = pl->ran_bwd_pipe = pipe;
    pl->launches = 1;
    pl->slabs = imin((M + PB - 1) / PB, 1024);  // the grid: one slab per workgroup
    return MCP_OK;
  }
  memset(pl, 0, sizeof(*pl));
  return MCP_ERR_LIMIT;
}

}  // namespace mcp
