// Fused closed loop under a tanh multilayer perceptron for gfx950 (MI355X), and its reverse-time sweep: Policy.MLP_policy as MC_PILCO's
// control policy.  The policy is this project's own (the reference has no such class); the loop it closes is MC_PILCO.apply_policy's
// (policy_learning/MC_PILCO.py:615-674) over Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718).
//   mcp_rollout_mlp      M trajectories, T steps, ONE launch: u_t = mlp(x_t) computed in the kernel; with jac the record for the sweep
//   mcp_rollout_mlp_bwd  the sweep: g_x0 and one partial slab of parameter gradients per workgroup of 16 trajectories
//   mcp_rollout_mlp_meas, mcp_rollout_mlp_meas_bwd   the same pair with the network fed a simulated measurement of x_t (template PMS:
//                        MC_PILCO4PMS.apply_policy, policy_learning/MC_PILCO.py:808-906, as mcp_rollout_pd_meas has it for the PD law)
//   mcp_rollout_mlp_drop, mcp_rollout_mlp_drop_bwd   either pair with inverted dropout on the hidden units (template DROP; masks from the
//                        launch's mcp_noise: a buffer, or Philox on the RBF masks' stream); p_drop == 0: the kernels without DROP
//   mcp_rollout_mlp_track, mcp_rollout_mlp_track_bwd   the dropout pair with target-trajectory features behind the network's own (template TRK:
//                        the errors target[t][idx[i]] - x[idx[i]], the map of policy_learning/Policy.py:389-403); no track: the dropout pair
//   mcp_rollout_mlp_res, mcp_rollout_mlp_res_bwd   the tracking pair with a PD term added to the network's output ahead of the squashing (template
//                        RES: PD_controller's law, policy_learning/Policy.py:406-449, and the network as its correction); no term: the tracking pair
// The forward kernel is the step loop of rollout_open.hip's feedback form with the PD law exchanged for the network: phases S, K, V, J, J', F
// and the noise addressing are the same functions (rollout_open_phases.h) and the same statements on the same operands, and the library is
// built without floating-point contraction, so the states carry the bits of mcp_rollout_open fed with the launch's own inputs.  Per step
// and tile of PT trajectories the network adds, behind the barrier that publishes x_t:
//   features   thread (trajectory, feature source): x[non_angle] as it is, one sincos_fast per angle          [PT][P]  in LDS
//   layer l    thread (trajectory, unit), PT * width dot products dealt over the 512 threads, fast_tanh        [PT][h_l] in LDS
//   output     the threads that fetch the inputs in the open-loop form: dot product, squashing, inputs[t], z
// one LDS barrier behind each.  The weights are launch constants: copied to LDS once (rows at an odd pitch: a wave reads one column of
// a layer without bank conflicts) where they fit beside the step's layout, else read from global memory (L2) in every step.
// (This header: the kernel templates, their argument structs, the descriptor checks and the launch ladders; rollout_mlp.hip: the dispatchers and
// the C entries, which instantiate every form but the history forms; rollout_mlp_hist.hip: the history forms.)
#pragma once
#include "rollout_open_phases.h"

using namespace mcp;

// ---- the network's geometry: layers in order (the output layer is the descriptor's slot 2), parameter offsets of g_params, LDS copy ----
struct MlpGeom {
  int nl;                   // layers, hidden + 1
  int in[3], out[3];        // widths
  int woff[3], boff[3];     // offsets in the parameter order W0 | b0 | [W1 | b1] | Wout | bout
  int pitch[3], wl[3], bl[3];  // LDS copy: row pitch (in | 1), offsets of the weights and biases
  int nparam, lds;
};
__host__ __device__ inline MlpGeom mlp_geom(const mcp_mlp_policy& p) {
  MlpGeom g;
  g.nl = p.n_hidden + 1;
  int o = 0, lo = 0, in = p.P;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int out = l >= g.nl ? 0 : (l < p.n_hidden ? p.h[l] : p.U);
    g.in[l] = l >= g.nl ? 0 : in;
    g.out[l] = out;
    g.woff[l] = o;
    o += out * g.in[l];
    g.boff[l] = o;
    o += out;
    g.pitch[l] = g.in[l] | 1;
    g.wl[l] = lo;
    lo += out * g.pitch[l];
    g.bl[l] = lo;
    lo += out;
    in = out;
  }
  g.nparam = o;
  g.lds = (lo + 1) & ~1;
  return g;
}
__host__ __device__ inline int mlp_slot(const mcp_mlp_policy& p, int l) { return l < p.n_hidden ? l : 2; }  // layer l in the descriptor

// copies the weights to LDS at the padded pitch (every thread of the workgroup; the caller's barrier follows)
__device__ __forceinline__ void mlp_stage_weights(const mcp_mlp_policy& p, const MlpGeom& g, double* wl, int tid, int nt) {
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    if (l >= g.nl) break;
    const double* W = p.W[mlp_slot(p, l)];
    const double* b = p.b[mlp_slot(p, l)];
    const int in = g.in[l], n = g.out[l] * in;
    for (int it = tid; it < n; it += nt) {
      const int j = it / in, i = it - j * in;
      wl[g.wl[l] + j * g.pitch[l] + i] = W[it];
    }
    for (int j = tid; j < g.out[l]; j += nt) wl[g.bl[l] + j] = b[j];
  }
}

// pre-activation of unit j on the input row x: the bias first, then the row's products in order -- the ONE order of operations of the
// forward kernel and of the sweep's recomputation
__device__ __forceinline__ double mlp_unit(const double* wr, double bias, const double* x, int in) {
  double acc = bias;
  for (int i = 0; i < in; ++i) acc = fma(wr[i], x[i], acc);
  return acc;
}

// ---- forward (template WLDS: the weights have an LDS copy; a form keeps only the addresses of the copy it reads) ----------------------------
struct OpenArgsMlp : OpenArgs {
  mcp_mlp_policy mlp;  // (the index lists normalised by the host: without lists non_angle = 0 .. S - 1)
  double* inputs;      // [T][M][U]
};
// MEASURED form (template PMS, mcp_rollout_mlp_meas): the network reads a simulated measurement y_t of x_t -- rollout_open.hip's measured
// feedback form with the PD law exchanged for the network.  The measurement is that form's statements, the same operations in the same order
// (stated here a second time: as a function shared through rollout_open_phases.h they moved the register figures of rollout_open.hip's own
// measured forms): the state thread of a measured position keeps np, nv, mv of its pair in registers and writes y[p],
// y[v] into the row [PT][S] at L.ym; the noise addressing is the closed-loop kernels'.  The feature threads read that row instead of xs behind
// the barrier that already publishes x_t: no barrier is added, and phases K, V, J, F see the operands they see without a measurement.
struct OpenArgsMlpMeas : OpenArgsMlp {
  mcp_meas ms;
};
template <bool PMS>
struct MlpArgsOf {
  typedef OpenArgsMlp type;
};
template <>
struct MlpArgsOf<true> {
  typedef OpenArgsMlpMeas type;
};
struct MlpActs {
  int fp, hp[2];       // row pitches of the features and of the hidden layers (odd)
  int f, h[2], w, total;  // offsets inside the form's region of the layout
};
__host__ __device__ inline MlpActs mlp_acts(int PT, const mcp_mlp_policy& p, const MlpGeom& g, bool wlds) {
  MlpActs A;
  int o = 0;
  A.fp = p.P | 1;
  A.f = o, o += PT * A.fp;
#pragma unroll
  for (int l = 0; l < 2; ++l) {
    A.hp[l] = (l < p.n_hidden ? p.h[l] : 0) | 1;
    A.h[l] = o;
    o += l < p.n_hidden ? PT * A.hp[l] : 0;
  }
  o = (o + 1) & ~1;
  A.w = o;
  A.total = o + (wlds ? g.lds : 6);  // (no copy: the six addresses of the weights, read from LDS in the loop -- they then cost no scalar registers)
  return A;
}

template <int PT>
__device__ __forceinline__ void mlp_layer_fwd(const double* W, const double* b, int pitch, int in, int out, const double* x, int xp, double* y, int yp,
                                              int tid) {
  for (int it = tid; it < PT * out; it += RF_NT) {
    const int p = it / out, j = it - p * out;
    y[p * yp + j] = fast_tanh(mlp_unit(W + j * pitch, b[j], x + p * xp, in));
  }
}

// DROPOUT form (template DROP, mcp_rollout_mlp_drop): inverted dropout on the hidden units, behind the activation --
//   h_l[j] = keep[t][m][off_l + j] ? tanh(pre_l[j]) / (1 - p) : 0,   off_0 = 0, off_1 = h[0],   H = h[0] (+ h[1])
// one row of H keep decisions per policy evaluation (row T - 1 included), as the RBF policy has one of B: the launch's mask buffer
// [T][M][H] where it has one, else philox_keep -- the RBF kernels' function and stream -- with the unit's index off_l + j in the basis
// function's place (a Philox block of four may so serve units of both layers).  The decision is made by the thread that owns
// (trajectory, unit); features, the output layer and the squashing are never dropped.  The forms without DROP take no part in any of it.
struct MlpDropArgs {
  uint32_t thr;          // drop_threshold(p)
  double scale, keep_p;  // 1 / (1 - p), 1 - p
};
template <bool PMS>
struct OpenArgsMlpDrop : MlpArgsOf<PMS>::type {
  MlpDropArgs drop;
};
// TRACKING form (template TRK, mcp_rollout_mlp_track): n more feature sources per trajectory -- source nnp + nap + i reads component idx[i]
// of the row the other sources read (xs; measured form: the measurement row) and of target[t], and writes the error target - x behind the
// cosines, at nnp + 2 nap + i.  At most 2 * MCP_MAX_STATE sources in all (the two lists are disjoint): with PT = 16 exactly the RF_NT threads.
// The target is read from global memory at the top of the step, ahead of the barrier that publishes x_t.  The tracking forms are built on the
// dropout forms' arguments and statements alone (p_drop == 0: `nodrop`, every unit kept at scale 1 -- the bits of the forms without
// dropout -- and neither masks nor Philox are looked at); the forms without TRK take no part in any of it.
struct MlpTrackArgs {
  int n, nodrop;
  int idx[MCP_MAX_STATE];
  const double* target;  // [rows >= T][S]
};
static_assert(2 * MCP_MAX_STATE * 16 <= RF_NT, "a feature source per thread in the widest tile");
template <bool PMS>
struct OpenArgsMlpTrack : OpenArgsMlpDrop<PMS> {
  MlpTrackArgs trk;
};
// RESIDUAL form (template RES, mcp_rollout_mlp_res): the PD law's term joins the network's output ahead of the one squashing,
//   av = a_mlp + (kp2 * ep + kd2 * ev),   kp2 = sqrt_kp[k]^2, kd2 = sqrt_kd[k]^2 (squared once per launch, as rollout_open.hip's PD kernel),
//   ep = target[t][pos[k]] - x[pos[k]],  ev = target[t][vel[k]] - x[vel[k]]
// in the output thread of (trajectory, k): x is the row the feature threads read (xs; measured form: the measurement row), still standing
// behind the layers' barriers, and the two entries of target[t] are asked for at the top of the step, beside tgv: no barrier is added.
// Dropout never touches the term.  The residual forms are built on the tracking forms' arguments and statements (trk.n == 0 and p_drop == 0
// are legal there); the forms without RES take no part in any of it.
struct MlpResArgs {
  int pos[MCP_MAX_INPUT], vel[MCP_MAX_INPUT];
  const double* sqrt_kp;
  const double* sqrt_kd;
  const double* target;  // [rows >= T][S]
};
template <bool PMS>
struct OpenArgsMlpRes : OpenArgsMlpTrack<PMS> {
  MlpResArgs res;
};
// HISTORY form (template HIST, mcp_rollout_mlp_hist): the feature row holds hist blocks of the network's own features, the newest first,
//   f_t = [phi(r_t), phi(r_{t-1}), ..., phi(r_{t-hist+1}), errors_t],   r_{t-j} := r_0 for t - j < 0,   P = hist P0 + trk.n,  P0 = nnp + 2 nap
// (r_t the row the feature threads read, xs: the history forms have NO measured form, static_assert below).  The feature threads still compute ONE block per step,
// phi(r_t), into block 0 -- at t = 0 into every block -- and the errors behind the last block.  The window is the feature row itself (the
// region `extra` of open_layout grows by PT (hist - 1) P0 doubles through P): behind the barrier that ends layer 0, the row's only reader,
// thread (trajectory, column i < P0) moves its column one block down, oldest first -- block j <- block j - 1, j = hist - 1 .. 1 -- PT (hist
// - 1) P0 moves in all; a column has one thread, so the moves need no barrier among themselves, and the barriers that already stand between
// layer 0 and the next step's feature stage publish them: NO barrier is added.  Layer 0 sees one contiguous row [PT][P | 1] and mlp_unit keeps
// its one order of operations.  (A rotating base with a two-segment dot product was the other way: it saves the moves -- at most 16 x 3 x 32
// LDS copies on 512 threads, three per thread -- and costs layer 0 a second loop and a run-time split in every unit of every step; the
// moves were chosen.)  The history forms are built on the residual forms' arguments and statements (trk.n == 0, the PD term off and
// p_drop == 0 are legal there); the forms without HIST take no part in any of it.
template <bool PMS>
struct OpenArgsMlpHist : OpenArgsMlpRes<PMS> {
  int hist;    // 2 .. MCP_MAX_HIST
  int res_on;  // the PD term: on (else its gains are zero and its target rows are not read)
};
template <bool PMS, bool DROP, bool TRK = false, bool RES = false, bool HIST = false>
struct MlpKernelArgs {
  typedef typename MlpArgsOf<PMS>::type type;
};
template <bool PMS>
struct MlpKernelArgs<PMS, true, false, false, false> {
  typedef OpenArgsMlpDrop<PMS> type;
};
template <bool PMS>
struct MlpKernelArgs<PMS, true, true, false, false> {
  typedef OpenArgsMlpTrack<PMS> type;
};
template <bool PMS>
struct MlpKernelArgs<PMS, true, true, true, false> {
  typedef OpenArgsMlpRes<PMS> type;
};
template <bool PMS>
struct MlpKernelArgs<PMS, true, true, true, true> {
  typedef OpenArgsMlpHist<PMS> type;
};
// whether unit `unit` of trajectory m (of this launch's M; the descriptor adds particle_offset) is kept in row t
__device__ __forceinline__ bool mlp_keep(const mcp_noise& nzl, uint32_t thr, int H, int M, int m, int t, int unit) {
  return nzl.masks ? nzl.masks[((size_t)t * M + m) * H + unit] != 0 : philox_keep(nzl, m, t, unit, thr);
}
template <int PT>
__device__ __forceinline__ void mlp_layer_fwd_drop(const double* W, const double* b, int pitch, int in, int out, const double* x, int xp, double* y,
                                                   int yp, int tid, const mcp_noise& nzl, const MlpDropArgs& dr, int H, int off, int M, int m0, int t,
                                                   bool all = false) {  // (all: a tracking form without dropout -- every unit kept)
  for (int it = tid; it < PT * out; it += RF_NT) {
    const int p = it / out, j = it - p * out;
    const bool keep = all || mlp_keep(nzl, dr.thr, H, M, imin(m0 + p, M - 1), t, off + j);
    const double h = fast_tanh(mlp_unit(W + j * pitch, b[j], x + p * xp, in));
    y[p * yp + j] = keep ? dr.scale * h : 0.0;
  }
}

template <int PT, int MAXDEG, bool NEEDVAR, bool NEEDJAC, bool WLDS, bool PMS = false, bool DROP = false, bool TRK = false, bool RES = false,
          bool HIST = false>
__global__ __launch_bounds__(RF_NT) void rollout_mlp_kernel(typename MlpKernelArgs<PMS, DROP, TRK, RES, HIST>::type a) {
  static_assert(DROP || !TRK, "the tracking forms are built on the dropout forms");
  static_assert(TRK || !RES, "the residual forms are built on the tracking forms");
  static_assert(RES || !HIST, "the history forms are built on the residual forms");
  static_assert(!(PMS && HIST), "the history forms have no measured form");
  extern __shared__ double smem[];
  const mcp_model& md = a.model;
  const mcp_mlp_policy& pl = a.mlp;
  const int S = md.S, U = md.U, G = md.G, D = md.D, M = a.M, T = a.T;
  const int nna = md.n_not_angle, na = md.n_angle;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const MlpGeom mg = mlp_geom(pl);
  const MlpActs A = mlp_acts(PT, pl, mg, WLDS);
  const OpenLayout L = open_layout(PT, NEEDVAR, S, D, G, a.NpadMax, NEEDJAC, a.na, PMS, A.total);
  double* xs = smem + L.xs;
  double* z = smem + L.z;
  double* red = smem + L.red;  // [2][G][RF_NW][PT]
  GpL* gpl = reinterpret_cast<GpL*>(smem + L.gpl);
  double* kpar = smem + L.kpar;
  double* panel = smem + L.panel;
  double* vpan = smem + L.vpan;  // (recording form)
  double* wjl = smem + L.wj;
  double* redj = smem + L.redj;
  double* fl = smem + L.ext + A.f;       // features [PT][fp]
  double* hl0 = smem + L.ext + A.h[0];   // hidden layers [PT][hp]
  double* hl1 = smem + L.ext + A.h[1];
  double* wlc = smem + L.ext + A.w;      // the weights' LDS copy
  const mcp_noise nzl = noise_of_launch(a.nz);
  const int m0 = blockIdx.x * PT;

  stage_gp_tables(md.gp, md.var_scale, G, D, gpl, kpar, tid);
  if (WLDS) mlp_stage_weights(pl, mg, wlc, tid, RF_NT);
  const double** wtab = reinterpret_cast<const double**>(wlc);  // (WLDS false) W[0..2] | b[0..2]
  if (!WLDS && tid < 6) wtab[tid] = tid < 3 ? pl.W[tid] : pl.b[tid - 3];
  if (L.xl) {  // mean mode: the small operands of phase K come from LDS for the whole launch
    const int NP = a.NpadMax;
    for (int g = 0; g < G; ++g) {
      const mcp_gp& gp = md.gp[g];
      for (int it = tid; it < D * NP; it += RF_NT) {
        const int d = it / NP, j = it - d * NP;
        smem[L.xt + (g * D + d) * NP + j] = j < gp.Npad ? gp.Xt[(size_t)d * gp.Npad + j] : 0.0;
      }
      for (int j = tid; j < NP; j += RF_NT) smem[L.al + g * NP + j] = j < gp.Npad ? gp.alpha[j] : 0.0;
    }
  }
  __syncthreads();
  // thread (p, s) owns state component s of trajectory p of the tile; the next PT * U threads compute the inputs
  const bool own = tid < PT * S;
  const int op = own ? tid / S : 0, os = own ? tid - op * S : 0;
  const int ut = tid - PT * S;
  const bool isu = ut >= 0 && ut < PT * U;
  const int up = isu ? ut / U : 0, uk = isu ? ut - up * U : 0;
  const int tp = own ? op : up;
  const int om = imin(m0 + tp, M - 1);
  const bool ovalid = m0 + tp < M;
  double xn = own ? a.x0[(size_t)om * S + os] : 0.0;
  int zi_plain = -1, zi_ang = -1, g_vel = -1, g_pos = -1, vel_of_pos = 0;
  if (own) {
    for (int i = 0; i < nna; ++i)
      if (md.not_angle[i] == os) zi_plain = i;
    for (int i = 0; i < na; ++i)
      if (md.angle[i] == os) zi_ang = i;
    for (int g = 0; g < G; ++g) {
      if (md.vel[g] == os) g_vel = g;
      if (md.not_vel[g] == os) {
        g_pos = g;
        vel_of_pos = md.vel[g];
      }
    }
  }
  const int og = g_pos >= 0 ? g_pos : g_vel;  // the GP whose increment this component integrates
  const double Ts = md.Ts;
  unsigned bad = 0;
  int cur = 0;
  // the network: thread (trajectory fq, feature source fi) of the feature stage; the output threads' bound
  int ntr = 0;         // (tracking form: the error sources behind the two lists' -- at most PT * nsrc = RF_NT threads, launch_mlp_w looks)
  bool alldrop = false;  // (and whether it runs without dropout)
  if constexpr (TRK) ntr = a.trk.n, alldrop = a.trk.nodrop != 0;
  (void)alldrop;
  const int nnp = pl.n_non_angle, nap = pl.n_angle, nsrc = nnp + nap + ntr;
  const bool isf = tid < PT * nsrc;
  const int fq = isf ? tid / nsrc : 0, fi = isf ? tid - fq * nsrc : 0;
  int fsrc = fi < nnp ? pl.non_angle[fi] : pl.angle[TRK ? imin(fi - nnp, MCP_MAX_STATE - 1) : fi - nnp];
  bool iserr = false;
  if constexpr (TRK) {
    iserr = isf && fi >= nnp + nap;
    if (iserr) fsrc = a.trk.idx[fi - nnp - nap];
  }
  const double umax = isu ? pl.u_max[uk] : 1.0;
  // (residual form) the output thread's PD term: its two components, its gains squared, its two entries of the PD target's row t (declared
  // here, outside the loop: a declaration inside it, dead as it is without RES, moved the spilled scalars of a tracking form)
  int rpos = 0, rvel = 0;
  double kp2 = 0.0, kd2 = 0.0, tgp = 0.0, tgq = 0.0;
  if constexpr (HIST) {  // (a history form may run without the PD term: its output threads then take no part in it)
    if (isu && a.res_on) {
      const double kp = a.res.sqrt_kp[uk], kd = a.res.sqrt_kd[uk];
      rpos = a.res.pos[uk], rvel = a.res.vel[uk];
      kp2 = kp * kp;
      kd2 = kd * kd;
    }
  } else if constexpr (RES) {
    if (isu) {
      const double kp = a.res.sqrt_kp[uk], kd = a.res.sqrt_kd[uk];
      rpos = a.res.pos[uk], rvel = a.res.vel[uk];
      kp2 = kp * kp;
      kd2 = kd * kd;
    }
  }
  (void)rpos, (void)rvel, (void)kp2, (void)kd2, (void)tgp, (void)tgq;
  // (history form) the blocks of the window, the width of one, and the mover of column hcol of trajectory hq
  int nhist = 1, P0 = 0, hq = 0, hcol = 0;
  bool ismv = false;
  if constexpr (HIST) {
    nhist = a.hist, P0 = nnp + 2 * nap;
    ismv = tid < PT * P0;
    hq = ismv ? tid / P0 : 0, hcol = ismv ? tid - hq * P0 : 0;
  }
  (void)nhist, (void)P0, (void)hq, (void)hcol, (void)ismv;
  const int nh = pl.n_hidden, H0 = pl.h[0], H1 = nh > 1 ? pl.h[1] : 0;
  const int HL = nh > 1 ? H1 : H0;                // the last hidden layer: its width, row pitch and rows
  const int hpL = nh > 1 ? A.hp[1] : A.hp[0];
  const double* hlL = nh > 1 ? hl1 : hl0;
  // (the output layer's place in the LDS copy, picked here: no table is indexed by a run-time layer number inside the loop)
  const int wlo = nh > 1 ? mg.wl[2] : mg.wl[1], blo = nh > 1 ? mg.bl[2] : mg.bl[1], pto = nh > 1 ? mg.pitch[2] : mg.pitch[1];
  // measured form: the pair of this state component (as in rollout_open_kernel)
  int pm_pos = -1, pm_vel = -1, pm_vc = 0;
  double pm_std = 0.0, pm_np = 0.0, pm_nv = 0.0, pm_mv = 0.0;
  if constexpr (PMS) {
    if (own) {
      for (int i = 0; i < a.ms.n; ++i) {
        if (a.ms.vel[i] == os) pm_vel = i;
        if (a.ms.pos[i] == os) {
          pm_pos = i;
          pm_vc = a.ms.vel[i];
          pm_std = a.ms.std_pos[i];
        }
      }
      if (pm_pos >= 0) pm_nv = pm_mv = a.x0[(size_t)om * S + pm_vc];
    }
  }
  lds_barrier();

  for (int t = 0; t < T; ++t) {
    double tgv = 0.0;  // (tracking form) this error source's component of target[t]: asked for here, needed behind the barrier
    if constexpr (TRK) {
      if (iserr) tgv = a.trk.target[(size_t)t * S + fsrc];
    }
    if constexpr (HIST) {
      if (isu && a.res_on) tgp = a.res.target[(size_t)t * S + rpos], tgq = a.res.target[(size_t)t * S + rvel];
    } else if constexpr (RES) {  // the output thread's two entries of the PD target's row t: asked for here as well
      if (isu) tgp = a.res.target[(size_t)t * S + rpos], tgq = a.res.target[(size_t)t * S + rvel];
    }
    // ---- phase S: publish x_t ----------------------------------------------------------------------------------------
    if (own) {
      xs[cur * PT * S + op * S + os] = xn;
      if (ovalid) {
        a.states[((size_t)t * M + m0 + op) * S + os] = xn;
        if (is_bad(xn)) bad |= MCP_STATUS_NAN;
      }
    }
    if constexpr (PMS) {  // y_t: the measurement of the row just formed (MC_PILCO.py:856-899)
      if (own && pm_vel < 0) {
        double* yr = smem + L.ym + op * S;
        double npos = xn, mv = 0.0;
        if (pm_pos >= 0) {
          if (t == 0) {
            mv = pm_mv;  // (row 0: the true velocity, which also starts both histories)
          } else {
            const double nn = a.ms.pos_noise ? a.ms.pos_noise[((size_t)(t - 1) * M + om) * a.ms.n + pm_pos]
                                             : philox_normal(nzl, om, t, pm_pos, MCP_STREAM_POS);
            npos = fma(pm_std, nn, xn);
            const double nv = (npos - pm_np) / Ts;
            mv = (a.ms.b0 * nv + a.ms.b1 * pm_nv - a.ms.a1 * pm_mv) / a.ms.a0;
            pm_nv = nv;
            pm_mv = mv;
          }
          pm_np = npos;
          yr[pm_vc] = mv;
        }
        yr[os] = npos;
        if (ovalid) {
          double* mr = a.ms.meas + ((size_t)t * M + m0 + op) * S;
          mr[os] = npos;
          if (pm_pos >= 0) mr[pm_vc] = mv;
          if (is_bad(npos) || is_bad(mv)) bad |= MCP_STATUS_NAN;
        }
      }
    }
    // ---- u_t = mlp(x_t) -- measured form: mlp(y_t) -- from the row just published (every row, the last one included: it is stored, and a
    // cost may read it).  The measurement row has one buffer: the feature threads read it here, its next writers are behind the barriers below
    lds_barrier();
    if (isf) {
      const double xv = PMS ? smem[L.ym + fq * S + fsrc] : xs[cur * PT * S + fq * S + fsrc];
      double* fr = fl + fq * A.fp;
      if constexpr (HIST) {  // block 0 of the window -- row 0: every block -- and the errors behind the last block
        const int nb = t == 0 ? nhist : 1;
        if (fi < nnp) {
          for (int j = 0; j < nb; ++j) fr[j * P0 + fi] = xv;
        } else if (!iserr) {
          double sn, cs;
          sincos_fast(xv, &sn, &cs);
          for (int j = 0; j < nb; ++j) fr[j * P0 + fi] = sn, fr[j * P0 + fi + nap] = cs;
        } else {
          fr[(nhist - 1) * P0 + fi + nap] = tgv - xv;  // (hist P0 + i, i = fi - nnp - nap)
        }
      } else if (fi < nnp) {
        fr[fi] = xv;
      } else if (!iserr) {
        double sn, cs;
        sincos_fast(xv, &sn, &cs);
        fr[fi] = sn;
        fr[fi + nap] = cs;
      } else {
        fr[fi + nap] = tgv - xv;  // (nnp + 2 nap + i, i = fi - nnp - nap; the sweep's workers repeat this statement)
      }
    }
    lds_barrier();
    if constexpr (DROP) {
      mlp_layer_fwd_drop<PT>(WLDS ? wlc + mg.wl[0] : wtab[0], WLDS ? wlc + mg.bl[0] : wtab[3], WLDS ? mg.pitch[0] : pl.P, pl.P, H0, fl, A.fp, hl0,
                             A.hp[0], tid, nzl, a.drop, H0 + H1, 0, M, m0, t, alldrop);
    } else if (WLDS) {
      mlp_layer_fwd<PT>(wlc + mg.wl[0], wlc + mg.bl[0], mg.pitch[0], pl.P, H0, fl, A.fp, hl0, A.hp[0], tid);
    } else {
      mlp_layer_fwd<PT>(wtab[0], wtab[3], pl.P, pl.P, H0, fl, A.fp, hl0, A.hp[0], tid);
    }
    lds_barrier();
    if constexpr (HIST) {  // layer 0 was the feature row's only reader: the window moves one block down, a thread per column, oldest first
      if (ismv) {
        double* fr = fl + hq * A.fp + hcol;
        for (int j = nhist - 1; j >= 1; --j) fr[j * P0] = fr[(j - 1) * P0];
      }
    }
    if (nh > 1) {
      if constexpr (DROP) {
        mlp_layer_fwd_drop<PT>(WLDS ? wlc + mg.wl[1] : wtab[1], WLDS ? wlc + mg.bl[1] : wtab[4], WLDS ? mg.pitch[1] : H0, H0, H1, hl0, A.hp[0], hl1,
                               A.hp[1], tid, nzl, a.drop, H0 + H1, H0, M, m0, t, alldrop);
      } else if (WLDS) {
        mlp_layer_fwd<PT>(wlc + mg.wl[1], wlc + mg.bl[1], mg.pitch[1], H0, H1, hl0, A.hp[0], hl1, A.hp[1], tid);
      } else {
        mlp_layer_fwd<PT>(wtab[1], wtab[4], H0, H0, H1, hl0, A.hp[0], hl1, A.hp[1], tid);
      }
      lds_barrier();
    }
    double ufb = 0.0;
    if (isu) {
      const double* hr = hlL + up * hpL;
      double av = WLDS ? mlp_unit(wlc + wlo + uk * pto, wlc[blo + uk], hr, HL)
                         : mlp_unit(wtab[2] + uk * HL, wtab[5][uk], hr, HL);
      if constexpr (HIST) {
        if (a.res_on) {
          const double* xr = PMS ? smem + L.ym + up * S : xs + cur * PT * S + up * S;
          const double ep = tgp - xr[rpos], ev = tgq - xr[rvel];
          av = av + (kp2 * ep + kd2 * ev);
        }
      } else if constexpr (RES) {  // the row the feature threads read: its next writer is behind the barriers below
        const double* xr = PMS ? smem + L.ym + up * S : xs + cur * PT * S + up * S;
        const double ep = tgp - xr[rpos], ev = tgq - xr[rvel];
        av = av + (kp2 * ep + kd2 * ev);
      }
      ufb = pl.squash ? umax * fast_tanh(av / umax) : av;
      if (ovalid) {
        a.inputs[((size_t)t * M + m0 + up) * U + uk] = ufb;
        if (is_bad(ufb)) bad |= MCP_STATUS_NAN;
      }
    }
    if (t + 1 >= T) continue;  // (uniform) the last row: no transition
    if (own) {
      double* zp = z + op * D;
      if (zi_plain >= 0) zp[zi_plain] = xn;
      if (zi_ang >= 0) {
        double sn, cs;
        sincos_fast(xn, &sn, &cs);
        zp[nna + zi_ang] = sn;
        zp[nna + na + zi_ang] = cs;
      }
    }
    if (isu) z[up * D + nna + 2 * na + uk] = ufb;
    lds_barrier();
    // ---- phases K (and V) per GP ---------------------------------------------------------------------------------------
    for (int g = 0; g < G; ++g) {
      const GpL gp = gpl[g];
      // X^T and alpha of GP g: their LDS copies (row pitch NpadMax) where the launch staged them, else global memory (the GP's own Npad)
      const double* Xt = L.xl ? smem + L.xt + g * D * a.NpadMax : gp.Xt;
      const double* al = L.xl ? smem + L.al + g * a.NpadMax : gp.alpha;
      open_phase_k<PT, MAXDEG, NEEDVAR>(gp, kpar + g * KP_STRIDE(D), D, z, panel, red + g * RF_NW * PT, tid, wv, lane, Xt, al,
                                        L.xl ? a.NpadMax : gp.Npad);
      if (NEEDJAC && !NEEDVAR)  // the mean chain: beta = alpha, nothing of phase K is needed -- no barrier in between
        open_phase_j<PT, MAXDEG, false>(gp, kpar + g * KP_STRIDE(D), D, z, nullptr, 0.0, redj + g * L.redj_gp, a.na, wv, lane, Xt, al,
                                        L.xl ? a.NpadMax : gp.Npad);
      if (NEEDVAR) {
        lds_barrier();
        const int Npad = __builtin_amdgcn_readfirstlane(gp.Npad);
        double q = 0.0;
        for (int I0 = 32 * wv; I0 < Npad; I0 += 32 * RF_NW) q += open_v_block<PT, NEEDJAC>(gp.Kinv, Npad, I0, panel, vpan, lane);
        q = fold_kk(q);
        if (lane < PT) red[(G + g) * RF_NW * PT + wv * PT + lane] = q;
        lds_barrier();  // the panel is rewritten by the next GP (recording form: by phase J's partial sums)
        if (NEEDJAC) {
          const int nn = (lane & 15) < PT ? (lane & 15) : 0;
          const double wjs = open_wjs<PT, MAXDEG>(a, nzl, gp, kpar + g * KP_STRIDE(D), D, G, g, t, imin(m0 + nn, M - 1), z + nn * D, red, nn);
          if (wv == 0 && lane < PT) wjl[lane] = wjs;
          open_phase_j<PT, MAXDEG, true>(gp, kpar + g * KP_STRIDE(D), D, z, vpan, wjs, redj, a.na, wv, lane, Xt, al, gp.Npad);
          lds_barrier();
          open_jac_store<PT, MAXDEG, true>(a, gp, kpar + g * KP_STRIDE(D), g, t, m0, z, wjl, redj, a.na, tid);
          lds_barrier();  // the next GP's phase K writes the panel again
        }
      }
    }
    if (!NEEDVAR) lds_barrier();
    if (NEEDJAC && !NEEDVAR)
      for (int g = 0; g < G; ++g) open_jac_store<PT, MAXDEG, false>(a, gpl[g], kpar + g * KP_STRIDE(D), g, t, m0, z, nullptr, redj + g * L.redj_gp, a.na, tid);
    // ---- phase F: moments, sample, integrate   v' = v + delta ;  q' = q + Ts v + Ts/2 delta   (Model_learning.py:711-716) ----
    if (own) {
      const double* xc = xs + cur * PT * S + op * S;
      double nx = 0.0;
      if (og >= 0) {
        const GpL& gp = gpl[og];
        const double* kp = kpar + og * KP_STRIDE(D);
        const double* zp = z + op * D;
        double mu = gp.mean;
#pragma unroll
        for (int w = 0; w < RF_NW; ++w) mu += red[og * RF_NW * PT + w * PT + op];
        double var = 0.0, dv = mu;
        if (NEEDVAR) {
          double ktv = 0.0;
#pragma unroll
          for (int w = 0; w < RF_NW; ++w) ktv += red[(G + og) * RF_NW * PT + w * PT + op];
          double kzz = gp.lambda;
          if (MAXDEG >= 1 && gp.deg >= 1) {
            double p1 = kp[KP_W1(D) + D];
            for (int d = 0; d < D; ++d) p1 = fma(kp[KP_W1(D) + d] * zp[d], zp[d], p1);
            kzz += p1;
            if (MAXDEG >= 2 && gp.deg >= 2) {
              double Sa = 0.0, Sb = 0.0;
              for (int d = 0; d < D; ++d) {
                const double zz = zp[d] * zp[d];
                Sa = fma(kp[KP_W20(D) + d], zz, Sa);
                Sb = fma(kp[KP_W21(D) + d], zz, Sb);
              }
              kzz = fma(Sa, Sb, kzz);
            }
          }
          var = (kzz - ktv) * gp.var_scale;
          if (a.sample) {
            const double e = nzl.eps ? nzl.eps[((size_t)t * M + om) * G + og] : philox_normal(nzl, om, t, og);
            dv = fma(sqrt(var), e, mu);
          }
        }
        if (og == g_vel && ovalid) {  // every GP has exactly one velocity component: its thread reports
          const size_t o = ((size_t)t * M + m0 + op) * G + og;
          if (a.mu) a.mu[o] = mu;
          if (NEEDVAR && a.var) a.var[o] = var;
          if (a.sample && var <= 0.0) bad |= MCP_STATUS_NONPOS_VAR;  // (finite and not positive: a NaN variance is MCP_STATUS_NAN)
          if (is_bad(mu) || is_bad(var)) bad |= MCP_STATUS_NAN;
        }
        nx = og == g_pos ? xc[os] + Ts * xc[vel_of_pos] + 0.5 * Ts * dv : xc[os] + dv;
      }
      xn = nx;
    }
    if ((NEEDVAR && MAXDEG >= 1) || NEEDJAC) lds_barrier();  // k(z, z) above (and phase J') read z, which the next step's phase S rewrites
    cur ^= 1;
  }
  if (bad) atomicOr(a.status, bad);
}

// ---- descriptor checks (host fields only: the weights are device memory) ------------------------------------------------------------------
// The precedence of pd_policy_check: a compiled limit first (MCP_ERR_LIMIT), then everything else (MCP_ERR_ARG).  n_hidden is looked at
// before the widths it counts.  `tr` (the track entries; NULL: none): its n is a compiled limit with the descriptor's and counts in P; its
// own errors come behind the descriptor's, T being the rows the launch reads of its target.  `hs` (the history entries; NULL: h = 1): h above
// MCP_MAX_HIST is a compiled limit with the descriptor's, h < 1 an argument error with its sizes', and h multiplies the network's own
// features in P.
static int mlp_policy_check(const mcp_model* model, const mcp_mlp_policy* p, const mcp_mlp_track* tr = nullptr, int T = 0,
                            const mcp_mlp_hist* hs = nullptr) {
  const int ntr = tr ? tr->n : 0, nh = hs ? hs->h : 1;
  if (p->U > MCP_MAX_INPUT || p->S > MCP_MAX_STATE || p->P > MCP_MAX_PFEAT || ntr > MCP_MAX_STATE || nh > MCP_MAX_HIST) return MCP_ERR_LIMIT;
  if (p->n_hidden < 1 || p->n_hidden > 2) return MCP_ERR_ARG;
  for (int l = 0; l < p->n_hidden; ++l)
    if (p->h[l] > MCP_MAX_HIDDEN) return MCP_ERR_LIMIT;
  if (p->n_angle > MCP_MAX_STATE || p->n_non_angle > MCP_MAX_STATE) return MCP_ERR_LIMIT;
  if (p->U < 1 || p->U != model->U || p->S != model->S || p->n_angle < 0 || p->n_non_angle < 0 || nh < 1) return MCP_ERR_ARG;
  for (int l = 0; l < p->n_hidden; ++l)
    if (p->h[l] < 1) return MCP_ERR_ARG;
  const bool lists = p->n_angle > 0 || p->n_non_angle > 0;
  if (p->P != nh * (lists ? p->n_non_angle + 2 * p->n_angle : p->S) + (ntr > 0 ? ntr : 0)) return MCP_ERR_ARG;
  unsigned seen = 0;  // an index at most once in the two lists together
  for (int i = 0; i < p->n_angle + p->n_non_angle; ++i) {
    const int s = i < p->n_angle ? p->angle[i] : p->non_angle[i - p->n_angle];
    if (s < 0 || s >= p->S || (seen >> s & 1u)) return MCP_ERR_ARG;
    seen |= 1u << s;
  }
  for (int l = 0; l <= p->n_hidden; ++l) {
    const int sl = l < p->n_hidden ? l : 2;
    if (!p->W[sl] || !p->b[sl]) return MCP_ERR_ARG;
  }
  for (int k = 0; p->squash && k < p->U; ++k)
    if (!(p->u_max[k] > 0.0)) return MCP_ERR_ARG;
  if (ntr < 0) return MCP_ERR_ARG;
  if (ntr > 0) {
    if (!tr->target || tr->rows < T) return MCP_ERR_ARG;
    unsigned errs = 0;  // an error feature per component at most
    for (int i = 0; i < ntr; ++i) {
      const int s = tr->idx[i];
      if (s < 0 || s >= p->S || (errs >> s & 1u)) return MCP_ERR_ARG;
      errs |= 1u << s;
    }
  }
  return MCP_OK;
}
// whether a track entry runs its tracking kernels (tr NULL or n == 0: the dropout entry's own kernels on the same arguments)
static inline bool track_active(const mcp_mlp_track* tr) { return tr && tr->n > 0; }
static MlpTrackArgs mlp_track_args(const mcp_mlp_track* tr, double p_drop) {
  MlpTrackArgs t;
  memset(&t, 0, sizeof(t));
  t.n = tr->n, t.nodrop = p_drop > 0.0 ? 0 : 1, t.target = tr->target;
  for (int i = 0; i < tr->n; ++i) t.idx[i] = tr->idx[i];
  return t;
}
// The PD term of the residual entries (res NULL or on == 0: none), behind the descriptor's and the track's checks: T the rows the launch
// reads of its target.  (More than MCP_MAX_INPUT inputs is a limit of the model, refused before.)
static inline bool res_active(const mcp_mlp_pd* res) { return res && res->on != 0; }
static int mlp_res_check(const mcp_mlp_policy* p, const mcp_mlp_pd* res, int T) {
  if (!res_active(res)) return MCP_OK;
  unsigned seenp = 0, seenv = 0;
  for (int k = 0; k < p->U; ++k) {
    const int sp = res->pos[k], sv = res->vel[k];
    if (sp < 0 || sp >= p->S || sv < 0 || sv >= p->S) return MCP_ERR_ARG;
  }
  for (int k = 0; k < p->U; ++k) {
    const int sp = res->pos[k], sv = res->vel[k];
    if ((seenp >> sp & 1u) || (seenv >> sv & 1u)) return MCP_ERR_ARG;
    seenp |= 1u << sp, seenv |= 1u << sv;
  }
  if (!res->sqrt_kp || !res->sqrt_kd || !res->target) return MCP_ERR_ARG;
  if (res->rows < T) return MCP_ERR_ARG;
  return MCP_OK;
}
static MlpResArgs mlp_res_args(const mcp_mlp_pd* res) {
  MlpResArgs r;
  memset(&r, 0, sizeof(r));
  for (int k = 0; k < MCP_MAX_INPUT; ++k) r.pos[k] = res->pos[k], r.vel[k] = res->vel[k];
  r.sqrt_kp = res->sqrt_kp, r.sqrt_kd = res->sqrt_kd, r.target = res->target;
  return r;
}
// the track a residual form runs on: the caller's, or one without errors
static MlpTrackArgs mlp_track_args_or_none(const mcp_mlp_track* tr, double p_drop) {
  if (tr && tr->n > 0) return mlp_track_args(tr, p_drop);
  MlpTrackArgs t;
  memset(&t, 0, sizeof(t));
  t.nodrop = p_drop > 0.0 ? 0 : 1;
  return t;
}
// the descriptor the kernels see: without lists the features are the state
static mcp_mlp_policy mlp_normalised(const mcp_mlp_policy* p) {
  mcp_mlp_policy q = *p;
  if (q.n_angle == 0 && q.n_non_angle == 0) {
    q.n_non_angle = q.S;
    for (int s = 0; s < q.S; ++s) q.non_angle[s] = s;
  }
  if (q.n_hidden == 1) q.h[1] = 0, q.W[1] = q.b[1] = nullptr;
  return q;
}

// ---- host path of the forward entry: checks -> fill -> ladder -----------------------------------------------------------------------------
// one rung: the weights in LDS where the layout then fits, else in global memory; MCP_ERR_LIMIT where the rung does not fit at all
template <int PT, int MAXDEG, bool NEEDVAR, bool NEEDJAC, bool WLDS, bool PMS, bool DROP, bool TRK = false, bool RES = false, bool HIST = false>
static int launch_mlp_w(const typename MlpKernelArgs<PMS, DROP, TRK, RES, HIST>::type& a, hipStream_t st) {
  const MlpActs A = mlp_acts(PT, a.mlp, mlp_geom(a.mlp), WLDS);
  const OpenLayout L = open_layout(PT, NEEDVAR, a.model.S, a.model.D, a.model.G, a.NpadMax, NEEDJAC, a.na, PMS, A.total);
  const size_t lds = (size_t)L.total * sizeof(double);
  if (lds > MCP_LDS_LIMIT) return MCP_ERR_LIMIT;
  if constexpr (TRK) {  // a thread per feature source (not reached within the compiled limits: the lists are disjoint, n <= MCP_MAX_STATE)
    if (PT * (a.mlp.n_non_angle + a.mlp.n_angle + a.trk.n) > RF_NT) return MCP_ERR_LIMIT;
  }
  MCP_ENSURE_MAX_LDS((rollout_mlp_kernel<PT, MAXDEG, NEEDVAR, NEEDJAC, WLDS, PMS, DROP, TRK, RES, HIST>));
  hipLaunchKernelGGL((rollout_mlp_kernel<PT, MAXDEG, NEEDVAR, NEEDJAC, WLDS, PMS, DROP, TRK, RES, HIST>), dim3((a.M + PT - 1) / PT), dim3(RF_NT), lds, st, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
template <int PT, int MAXDEG, bool NEEDVAR, bool NEEDJAC, bool PMS, bool DROP, bool TRK = false, bool RES = false, bool HIST = false>
static int launch_mlp(const typename MlpKernelArgs<PMS, DROP, TRK, RES, HIST>::type& a, hipStream_t st) {
  const int rc = launch_mlp_w<PT, MAXDEG, NEEDVAR, NEEDJAC, true, PMS, DROP, TRK, RES, HIST>(a, st);
  return rc == MCP_ERR_LIMIT ? launch_mlp_w<PT, MAXDEG, NEEDVAR, NEEDJAC, false, PMS, DROP, TRK, RES, HIST>(a, st) : rc;
}
template <int PT, bool NEEDVAR, bool NEEDJAC, bool PMS, bool DROP, bool TRK = false, bool RES = false, bool HIST = false>
static int launch_mlp_deg(const typename MlpKernelArgs<PMS, DROP, TRK, RES, HIST>::type& a, int maxdeg, hipStream_t st) {
  return maxdeg == 0 ? launch_mlp<PT, 0, NEEDVAR, NEEDJAC, PMS, DROP, TRK, RES, HIST>(a, st) : launch_mlp<PT, 2, NEEDVAR, NEEDJAC, PMS, DROP, TRK, RES, HIST>(a, st);
}
// The ladder of tiles of rollout_open.hip's launch_open_tiles (at every compiled limit at once the one-trajectory recording rung takes
// 85 KB + 1.3 KB of activations, the measured form one row [PT][S] more: nothing within the limits is refused), entered one rung lower
// by SMALL SWARMS: up to MLP_SMALL_SWARM trajectories start at 4 per workgroup.  Measured (profiles/NOTES.md part T): the time of a launch is the time of ONE tile's T steps for as
// long as every tile has a compute unit of its own, whatever M, and a tile of 4 takes 0.82x (UR5 shape) / 0.86x (arm shape) the time of a
// tile of 16 -- the Kinv stream and the MFMAs of phases V and J do not depend on the width, phase K does.  Tiles of 4 have a compute unit
// each up to M = 4 x 256 = 1024; at M = 1536 they take two rounds and twice the time, and tiles of 16 (96 workgroups) win again.  The tile
// width changes no bit of a trajectory (a column of phases K, V, J is computed the same way in every width: the identities with
// mcp_rollout_open hold across the rungs).
#define MLP_SMALL_SWARM 1024  // 4 trajectories x the 256 compute units of the MI355X
template <bool PMS, bool DROP = false, bool TRK = false, bool RES = false, bool HIST = false>
static int launch_mlp_tiles(const typename MlpKernelArgs<PMS, DROP, TRK, RES, HIST>::type& a, int maxdeg, bool wantvar, hipStream_t st) {
  const bool small = a.M <= MLP_SMALL_SWARM;
  if (!a.jac) {
    if (!a.sample && !wantvar) return launch_mlp_deg<1, false, false, PMS, DROP, TRK, RES, HIST>(a, maxdeg, st);
    int rc = small ? MCP_ERR_LIMIT : launch_mlp_deg<16, true, false, PMS, DROP, TRK, RES, HIST>(a, maxdeg, st);
    if (rc == MCP_ERR_LIMIT) rc = launch_mlp_deg<4, true, false, PMS, DROP, TRK, RES, HIST>(a, maxdeg, st);
    return rc;
  }
  if (!a.sample && !wantvar) return launch_mlp_deg<1, false, true, PMS, DROP, TRK, RES, HIST>(a, maxdeg, st);
  int rc = small ? MCP_ERR_LIMIT : launch_mlp_deg<16, true, true, PMS, DROP, TRK, RES, HIST>(a, maxdeg, st);
  if (rc == MCP_ERR_LIMIT) rc = launch_mlp_deg<4, true, true, PMS, DROP, TRK, RES, HIST>(a, maxdeg, st);
  if (rc == MCP_ERR_LIMIT) rc = launch_mlp_deg<1, true, true, PMS, DROP, TRK, RES, HIST>(a, maxdeg, st);
  return rc;
}

// the dropout probability of the _drop entries: looked at with the sizes (a NaN is refused)
static inline bool mlp_drop_ok(double p) { return p >= 0.0 && p < 1.0; }
static inline MlpDropArgs mlp_drop_args(double p) { return MlpDropArgs{drop_threshold(p), 1.0 / (1.0 - p), 1.0 - p}; }
// the arguments of a dropout form: those of the form without, and the probability's three numbers
template <class DropArgs, class Args>
static DropArgs mlp_with_drop(const Args& a, double p_drop) {
  DropArgs d;
  static_cast<Args&>(d) = a;
  d.drop = mlp_drop_args(p_drop);
  return d;
}

// the arguments of a tracking form: those of the dropout form (at any p_drop), and the track
template <class TrackArgs, class Args>
static TrackArgs mlp_with_track(const Args& a, double p_drop, const mcp_mlp_track* trk) {
  TrackArgs d = mlp_with_drop<TrackArgs, Args>(a, p_drop);
  d.trk = mlp_track_args(trk, p_drop);
  return d;
}

// the arguments of a residual form: those of the tracking form (with or without errors), and the PD term
template <class ResArgs, class Args>
static ResArgs mlp_with_res(const Args& a, double p_drop, const mcp_mlp_track* trk, const mcp_mlp_pd* res) {
  ResArgs d = mlp_with_drop<ResArgs, Args>(a, p_drop);
  d.trk = mlp_track_args_or_none(trk, p_drop);
  d.res = mlp_res_args(res);
  return d;
}

// the arguments of a history form: those of the residual form (with or without the PD term), and the depth of the window
static inline bool hist_active(const mcp_mlp_hist* hs) { return hs && hs->h > 1; }
template <class HistArgs, class Args>
static HistArgs mlp_with_hist(const Args& a, double p_drop, const mcp_mlp_track* trk, const mcp_mlp_pd* res, const mcp_mlp_hist* hs) {
  HistArgs d = mlp_with_drop<HistArgs, Args>(a, p_drop);
  d.trk = mlp_track_args_or_none(trk, p_drop);
  memset(&d.res, 0, sizeof(d.res));
  if (res_active(res)) d.res = mlp_res_args(res);
  d.hist = hs->h;
  d.res_on = res_active(res) ? 1 : 0;
  return d;
}

// ---------------------------------------------------------------------------------------
// Reverse-time sweep of the closed loop under the network: the open-loop sweep (rollout_open.hip: stages A, B, C, the loader wave) with
// the policy's stage between B and C.  Per row r and trajectory, with gu = gz[input slots] + g_inputs[r] (row T - 1: g_inputs alone):
//   abar = gu (1 - (u / u_max)^2)  (squash) or gu;   delta_out = abar;   delta_l = (W_{l+1}^T delta_{l+1}) (1 - h_l^2);   fbar = W_0^T delta_1
//   lambda[s] += fbar[i]  (s = non_angle[i])  |  cos x fbar[sin_i] - sin x fbar[cos_i]  (s = angle[i])                       (stage C)
//   g_W_l += delta_l h_{l-1}^T,  g_b_l += delta_l   summed over the rows and the tile's trajectories
// A workgroup of 8 waves owns 16 trajectories.  Wave 0 is the CHAIN (lane (p = l & 15, q = l >> 4): trajectory p, every fourth index) and
// carries only the delta back-propagation; wave 1 is the LOADER of the open-loop sweep.  Waves 2..7 are the WORKERS, off the chain:
//   activations  of row r - 1 while the chain runs row r: a wave per trajectory (lane = feature source, then lane = unit), recomputed from
//                states[r - 1] with the forward's order of operations (mlp_unit, fast_tanh, sincos_fast): the forward's bits
//   outer sums   of row r + 1, whose deltas the chain left in LDS one barrier ago: the n_param entries are dealt over the 384 worker
//                threads, at most MB_NACC each, held in registers across the whole sweep; a thread adds its entries' products over the
//                trajectories in order, row after row, and stores them once: the workgroup's slab
// Three rows of activations are alive at once (r + 1 read by the outer sums, r by the chain, r - 1 being written): three buffers, two of
// deltas, one workgroup barrier per row.  Where 16 trajectories of that do not fit the LDS the workgroup sweeps its 16 trajectories in
// parts of 8 / 4 / 2 / 1, one after the other, the sums staying in the registers: a slab is still one workgroup's.  No atomics; the order
// of every sum is fixed by the shape alone.
// MEASURED form (template PMS, mcp_rollout_mlp_meas_bwd): the forward's network read y_r (ms.meas), so the workers recompute the activations
// from ms.meas[r - 1] -- the forward's operands, the forward's bits -- and stage C takes fbar through the feature map at y_r: the policy's pull ON
// THE MEASUREMENT,   ybar_r[s] = fbar[i] (s = non_angle[i])  |  cos y fbar[sin_i] - sin y fbar[cos_i]  (s = angle[i]; sin y, cos y are the
// activation row's own entries, so no row of the measurement is held in LDS).  It reaches lambda through the adjoint of the filter exactly
// as in rollout_open_bwd_kernel<true, true> (rollout_open.hip): two carries per (trajectory, pair), zero behind the last row, kept in LDS at
// the pair's position component and zeroed at the start of every part (the same lane writes and reads them, row after row):
//   mvbar_r = ybar_r[v] - (a1/a0) mvbar_{r+1};   nvbar_r = (b0/a0) mvbar_r + (b1/a0) mvbar_{r+1}
//   r >= 1: lambda_r[p] += ybar_r[p] + (nvbar_r - nvbar_{r+1}) / Ts           (the true velocity of a later row gets nothing from the policy)
//   r == 0: lambda_0[p] += ybar_0[p] - nvbar_1 / Ts;   lambda_0[v] += ybar_0[v] + ((b1 - a1)/a0) mvbar_1         (row 0 is measured true)
// A component in no pair gets ybar_r[s] directly.  The slabs, the order of every sum and the parts are those of the plain form.
// ---------------------------------------------------------------------------------------
#define MB_PT 16
#define MB_NT 512
#define MB_NWORK (MB_NT - 128)  // worker threads
#define MB_NACC 18              // parameter entries per worker thread
static_assert(MCP_MAX_HIDDEN * (MCP_MAX_PFEAT + 1) + MCP_MAX_HIDDEN * (MCP_MAX_HIDDEN + 1) + MCP_MAX_INPUT * (MCP_MAX_HIDDEN + 1) + 2 * MCP_MAX_INPUT <=
                  MB_NACC * MB_NWORK,
              "a worker thread's share of the parameters (the residual form's two gain vectors included)");
#define MB_CMAX (MCP_MAX_HIDDEN / 4)  // columns per lane of the chain wave

struct MlpBwdArgs {
  int S, U, G, D, nna, na, M, T;
  int angle[MCP_MAX_STATE], not_angle[MCP_MAX_STATE], vel[MCP_MAX_GP], not_vel[MCP_MAX_GP];
  double Ts;
  const double* states;
  const double* inputs;
  const double* jac;
  const double* g_states;
  const double* g_inputs;  // or NULL
  double* g_x0;            // or NULL
  double* g_params;        // [ceil(M / 16)][n_param] or NULL
  mcp_mlp_policy mlp;      // (normalised)
  int pts;                 // trajectories per part: 16 / 8 / 4 / 2 / 1
  int wlds;
};

struct MlpBwdArgsMeas : MlpBwdArgs {
  mcp_meas ms;
};
template <bool PMS>
struct MlpBwdArgsOf {
  typedef MlpBwdArgs type;
};
template <>
struct MlpBwdArgsOf<true> {
  typedef MlpBwdArgsMeas type;
};

// DROPOUT form (template DROP, mcp_rollout_mlp_drop_bwd): the workers recompute the forward's keep decisions with the forward's function
// (mlp_keep, from the launch's noise descriptor) beside the activations -- a row holds the forward's h_l, zeros and scale included, so the
// outer sums need nothing more -- and leave the decisions of a row and trajectory as one ballot word per hidden layer; the chain tests its
// unit's bit: a dropped unit passes nothing, a kept one (1 - tanh^2) / (1 - p) with tanh = (1 - p) h.  Three rows of 2 words per trajectory.
template <bool PMS>
struct MlpBwdArgsDrop : MlpBwdArgsOf<PMS>::type {
  mcp_noise nz;
  MlpDropArgs drop;
};
// TRACKING form (template TRK, mcp_rollout_mlp_track_bwd; built on the dropout form, as the forward's): the workers recompute the error
// features of a row from the row the forward's network read and target[r] with the forward's statement (target - x), so the activation
// rows -- and through them the outer sums' columns of g_W0 -- carry the forward's bits; stage C takes the errors' pull
//   lambda[idx[i]] -= fbar[nnp + 2 nap + i]        (measured form: the same term in ybar, which reaches lambda through the filter's adjoint)
// from a table ferr[s] (the error feature of component s, or -1) beside fplain / fang, in a region of its own: the layouts of the forms
// without TRK do not move.
template <bool PMS>
struct MlpBwdArgsTrack : MlpBwdArgsDrop<PMS> {
  MlpTrackArgs trk;
};
// RESIDUAL form (template RES, mcp_rollout_mlp_res_bwd; built on the tracking form): with abar_k the adjoint of the output layer's
// pre-activation, which stage M leaves in LDS as delta_out[k],
//   lambda[pos[k]] -= sqrt_kp[k]^2 abar_k;   lambda[vel[k]] -= sqrt_kd[k]^2 abar_k          (stage C, tables kpos / kvel per state component and
//                                                                                             the squared gains in LDS; measured form: in ybar)
//   g_sqrt_kp[k] += 2 sqrt_kp[k] e[pos[k]] abar_k;   g_sqrt_kd[k] += 2 sqrt_kd[k] e[vel[k]] abar_k,   e = target[r] - x_r  (measured: y_r)
// The gain gradients are 2 U more entries of the workers' outer sums, behind bout: their delta is delta_out[k], their "activation" the
// factor 2 sqrt_k e, which the workers write behind the constant 1 of an activation row from the forward's operands, beside the error
// features.  So they stay off the chain wave, need no reduction of their own (the PD sweep's per-lane sums end in one), and the slab
// keeps its rule: one store per entry, a fixed order of sums.  The network's deltas are unchanged.
template <bool PMS>
struct MlpBwdArgsRes : MlpBwdArgsTrack<PMS> {
  MlpResArgs res;
};
// HISTORY form (template HIST, mcp_rollout_mlp_hist_bwd; built on the residual form, with or without its PD term): the activation row of
// row r holds the forward's feature row -- the workers recompute block j from row max(r - j, 0) of what the forward's network read, with
// the forward's functions, and the errors behind the last block -- so the outer sums' columns of g_W0 need nothing more.  The chain's fbar
// = W0^T delta_1 has P = hist P0 + n columns; block j of row r pulls on row max(r - j, 0) through the feature map AT THAT ROW, whose sines
// and cosines are block j of row r's own activation row.  So ahead of stage C the chain wave turns the blocks j >= 1 of fbar into pulls
// per state component at once (plain source i: fbar[j P0 + i]; angle source i: fbar[j P0 + nnp + i] cos - fbar[j P0 + nnp + nap + i] sin)
// and adds them, j ascending, into a ring pend[hist][pts][S] in LDS at slot max(r - j, 0) mod hist; stage C of row r' adds slot r' mod hist
// beside block 0's pull and the slot is cleared behind stage C.  Writer and reader of a slot's entry are the same lane (component s of
// trajectory p is lane (p, s mod 4)'s).  There is NO measured history form (static_assert in the kernel): one was written, faulted on the
// GPU at a timing shape, and was taken out with its cause not found; ybar knows nothing of the ring.  A
// slot is complete when its row reads it: its writers are the rows above (a workgroup barrier per row) and, for row 0's clamped blocks,
// this row's own pass, which a wave-level wait separates from stage C.  Row 0 collects the pull of every block that was clamped onto it.
// The order of every sum is fixed by the shape: two runs give the same bits.
template <bool PMS>
struct MlpBwdArgsHist : MlpBwdArgsRes<PMS> {
  int hist;    // 2 .. MCP_MAX_HIST
  int res_on;  // the PD term: on (else no gain gradients: slabs of n_param)
};
template <bool PMS, bool DROP, bool TRK = false, bool RES = false, bool HIST = false>
struct MlpBwdKernelArgs {
  typedef typename MlpBwdArgsOf<PMS>::type type;
};
template <bool PMS>
struct MlpBwdKernelArgs<PMS, true, false, false, false> {
  typedef MlpBwdArgsDrop<PMS> type;
};
template <bool PMS>
struct MlpBwdKernelArgs<PMS, true, true, false, false> {
  typedef MlpBwdArgsTrack<PMS> type;
};
template <bool PMS>
struct MlpBwdKernelArgs<PMS, true, true, true, false> {
  typedef MlpBwdArgsRes<PMS> type;
};
template <bool PMS>
struct MlpBwdKernelArgs<PMS, true, true, true, true> {
  typedef MlpBwdArgsHist<PMS> type;
};

struct MlpBwdLayout {
  int rec, xs, gs, lam, gd, gz, tab, ul, gul, fbar, act, del, w, total;  // offsets in doubles
  int car, mtab;               // measured form: the filter's carries | pvel, ppos
  int keep;                    // dropout form: the keep words [3][pts][2]
  int etab;                    // tracking form: ferr (ints, per state component)
  int ktab, gnl, res0;         // residual form: kpos | kvel (ints, per state component), sqrt_kp^2 | sqrt_kd^2; inside an activation row: 2 sqrt_k e
  int pend;                    // history form: the ring of pulls [hist][pts][S]
  int rp, fp, ap, dp;          // pitches: record row | fbar row | activation row | delta row (odd)
  int aoff[3], one, doff[3];   // inside an activation row: the input of layer l, the constant 1; inside a delta row: the output of layer l
};
__host__ __device__ inline MlpBwdLayout mlp_bwd_layout(int pts, int S, int U, int G, int D, const mcp_mlp_policy& p, const MlpGeom& g, bool wlds,
                                                       bool pms = false, bool drop = false, bool trk = false, bool res = false, int hist = 1) {
  MlpBwdLayout L;
  int o = 0;
  auto take = [&](int n) {
    int r = o;
    o += (n + 1) & ~1;
    return r;
  };
  L.rp = (G * D) | 1;
  L.fp = p.P | 1;
  int ao = 0, dd = 0;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    L.aoff[l] = ao;
    ao += g.in[l];
    L.doff[l] = dd;
    dd += g.out[l];
  }
  L.one = ao;
  L.res0 = ao + 1;
  L.ap = (ao + 1 + (res ? 2 * U : 0)) | 1;
  L.dp = dd | 1;
  L.rec = take(2 * pts * L.rp);
  L.xs = take(2 * pts * S);
  L.gs = take(2 * pts * S);
  L.lam = take(2 * pts * S);
  L.gd = take(pts * G);
  L.gz = take(pts * D);
  L.tab = take((7 * MCP_MAX_STATE + MB_PT) / 2 + 2);  // ints: og | ispos | velof | zplain | zang | fplain | fang (per state component), len (per trajectory)
  L.ul = take(2 * pts * U);
  L.gul = take(2 * pts * U);
  L.fbar = take(pts * L.fp);
  L.act = take(3 * pts * L.ap);
  L.del = take(2 * pts * L.dp);
  L.car = pms ? take(2 * pts * S) : 0;     // [trajectory][position component]: mvbar | nvbar of the row behind
  L.mtab = pms ? take(MCP_MAX_STATE) : 0;  // ints: pvel (per state component: the velocity of the pair it is the position of, or -1) | ppos (the converse)
  L.keep = drop ? take(3 * pts * 2) : 0;   // 64-bit words: bit j = unit j of hidden layer l of the row's trajectory is kept
  L.etab = trk ? take(MCP_MAX_STATE / 2) : 0;  // ints: ferr (per state component: the error feature that reads it, or -1)
  L.ktab = res ? take(MCP_MAX_STATE) : 0;      // ints: kpos | kvel (per state component: the input that reads it as position / velocity, or -1)
  L.gnl = res ? take(2 * MCP_MAX_INPUT) : 0;   // sqrt_kp^2 | sqrt_kd^2
  L.pend = hist > 1 ? take(hist * pts * S) : 0;  // the pulls of the blocks j >= 1 on the rows below, slot = row mod hist
  L.w = o;
  L.total = o + (wlds ? g.lds : 0);
  return L;
}

// chain wave: acc[i] = sum_k W[k][c_i] d[k] for this lane's columns c_i = q + 4 i < nin (W: nout rows at `pitch`)
__device__ __forceinline__ void mlp_back(const double* W, int pitch, int nin, int nout, const double* d, int q, double (&acc)[MB_CMAX]) {
  const int nc = (nin + 3) >> 2;
#pragma unroll
  for (int i = 0; i < MB_CMAX; ++i) acc[i] = 0.0;
  for (int k = 0; k < nout; ++k) {
    const double dk = d[k];
    const double* wr = W + k * pitch + q;
#pragma unroll
    for (int i = 0; i < MB_CMAX; ++i)
      if (i < nc) acc[i] = fma(q + 4 * i < nin ? wr[4 * i] : 0.0, dk, acc[i]);
  }
}

// the rows the forward's network read: the states, in the measured form the measurements
template <bool PMS>
__device__ __forceinline__ const double* mlp_policy_rows(const typename MlpBwdArgsOf<PMS>::type& a) {
  if constexpr (PMS) {
    return a.ms.meas;
  } else {
    return a.states;
  }
}

// the launch's noise descriptor of a dropout form (read once, as in the forward kernel); the other forms have none
template <bool PMS>
__device__ __forceinline__ mcp_noise mlp_bwd_noise(const MlpBwdArgsDrop<PMS>& a) {
  return noise_of_launch(a.nz);
}
template <bool PMS>
__device__ __forceinline__ mcp_noise mlp_bwd_noise(const MlpBwdArgsTrack<PMS>& a) {  // (built on the dropout form's arguments)
  return noise_of_launch(a.nz);
}
template <bool PMS>
__device__ __forceinline__ mcp_noise mlp_bwd_noise(const MlpBwdArgsRes<PMS>& a) {
  return noise_of_launch(a.nz);
}
template <bool PMS>
__device__ __forceinline__ mcp_noise mlp_bwd_noise(const MlpBwdArgsHist<PMS>& a) {
  return noise_of_launch(a.nz);
}
template <class Args>
__device__ __forceinline__ mcp_noise mlp_bwd_noise(const Args&) {
  return mcp_noise{};
}

template <bool WLDS, bool PMS = false, bool DROP = false, bool TRK = false, bool RES = false, bool HIST = false>
__global__ __launch_bounds__(MB_NT) void rollout_mlp_bwd_kernel(typename MlpBwdKernelArgs<PMS, DROP, TRK, RES, HIST>::type a) {
  static_assert(DROP || !TRK, "the tracking forms are built on the dropout forms");
  static_assert(TRK || !RES, "the residual forms are built on the tracking forms");
  static_assert(RES || !HIST, "the history forms are built on the residual forms");
  static_assert(!(PMS && HIST), "the history forms have no measured form: ybar below knows nothing of the ring");
  extern __shared__ double smem[];
  const mcp_mlp_policy& pl = a.mlp;
  const int S = a.S, U = a.U, G = a.G, D = a.D, M = a.M, T = a.T, nna = a.nna, na = a.na, pts = a.pts;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const MlpGeom mg = mlp_geom(pl);
  int nhist = 1;     // (history form: the blocks of the window; whether its PD term is on -- the residual forms always have theirs)
  bool pdon = RES;
  if constexpr (HIST) nhist = a.hist, pdon = a.res_on != 0;
  const MlpBwdLayout L = mlp_bwd_layout(pts, S, U, G, D, pl, mg, WLDS, PMS, DROP, TRK, RES, nhist);
  const int P0 = pl.n_non_angle + 2 * pl.n_angle;  // the width of one block
  double* pend = smem + L.pend;
  (void)P0, (void)pend, (void)pdon;
  int ntr = 0;           // (tracking form: the error features; whether it runs without dropout; ferr)
  bool alldrop = false;
  if constexpr (TRK) ntr = a.trk.n, alldrop = a.trk.nodrop != 0;
  (void)alldrop;
  int* ferr = reinterpret_cast<int*>(smem + L.etab);
  int* kpos = reinterpret_cast<int*>(smem + L.ktab);  // (residual form; so are the next two)
  int* kvel = kpos + MCP_MAX_STATE;
  double* gn2 = smem + L.gnl;
  int noterm = 0;  // (a history form without its PD term: no gain gradients in the slab)
  if constexpr (HIST) noterm = pdon ? 0 : 2 * U;
  const int ntot = mg.nparam + (RES ? 2 * U : 0) - noterm;  // the entries of a slab
  const int GD = G * D, RP = L.rp;
  double* rec = smem + L.rec;
  double* xsl = smem + L.xs;
  double* gsl = smem + L.gs;
  double* lam = smem + L.lam;
  double* gdl = smem + L.gd;
  double* gzl = smem + L.gz;
  int* ogt = reinterpret_cast<int*>(smem + L.tab);
  int* post = ogt + MCP_MAX_STATE;
  int* velof = post + MCP_MAX_STATE;
  int* zplain = velof + MCP_MAX_STATE;
  int* zang = zplain + MCP_MAX_STATE;
  int* fplain = zang + MCP_MAX_STATE;
  int* fang = fplain + MCP_MAX_STATE;
  int* lenl = fang + MCP_MAX_STATE;
  double* ull = smem + L.ul;
  double* gul = smem + L.gul;
  double* fbar = smem + L.fbar;
  double* act = smem + L.act;
  double* del = smem + L.del;
  double* car = smem + L.car;  // (measured form)
  int* pvel = reinterpret_cast<int*>(smem + L.mtab);
  int* ppos = pvel + MCP_MAX_STATE;
  double* wlc = smem + L.w;
  unsigned long long* kwl = reinterpret_cast<unsigned long long*>(smem + L.keep);  // (dropout form; so are the next two)
  const mcp_noise nzl = mlp_bwd_noise(a);
  const int Hd = pl.h[0] + pl.h[1];  // the width of a mask row (one hidden layer: h[1] = 0)
  const int nnp = pl.n_non_angle, nap = pl.n_angle, nl = mg.nl;
  // the weights as this kernel reads them (WLDS: the LDS copy, else global memory); the layer loops below are unrolled over the three
  // slots, so every index into these tables is a constant
  const double* Wl[3];
  const double* bl[3];
  int wp[3];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int sl = mlp_slot(pl, l);
    Wl[l] = WLDS ? wlc + mg.wl[l] : pl.W[sl];
    bl[l] = WLDS ? wlc + mg.bl[l] : pl.b[sl];
    wp[l] = WLDS ? mg.pitch[l] : mg.in[l];
  }
  const int dlast = nl == 3 ? L.doff[2] : L.doff[1];  // the output layer's deltas

  if (WLDS) mlp_stage_weights(pl, mg, wlc, tid, MB_NT);
  if (tid < S) {  // which GP a component integrates, as the forward kernel decides it; where it enters the two feature maps
    const int s = tid;
    int g_vel = -1, g_pos = -1, zp = -1, za = -1, fpl = -1, fan = -1;
    for (int g = 0; g < G; ++g) {
      if (a.vel[g] == s) g_vel = g;
      if (a.not_vel[g] == s) g_pos = g;
    }
    for (int i = 0; i < nna; ++i)
      if (a.not_angle[i] == s) zp = i;
    for (int i = 0; i < na; ++i)
      if (a.angle[i] == s) za = i;
    for (int i = 0; i < nnp; ++i)
      if (pl.non_angle[i] == s) fpl = i;
    for (int i = 0; i < nap; ++i)
      if (pl.angle[i] == s) fan = i;
    ogt[s] = g_pos >= 0 ? g_pos : g_vel;
    post[s] = g_pos >= 0 ? 1 : 0;
    velof[s] = g_pos >= 0 ? a.vel[g_pos] : -1;
    zplain[s] = zp;
    zang[s] = za;
    fplain[s] = fpl;
    fang[s] = fan;
    if constexpr (TRK) {
      int fe = -1;
      for (int i = 0; i < ntr; ++i)
        if (a.trk.idx[i] == s) fe = i;
      ferr[s] = fe;
    }
    if constexpr (RES) {
      int kp = -1, kv = -1;
      if constexpr (HIST) {
        for (int k = 0; k < (pdon ? U : 0); ++k) {
          if (a.res.pos[k] == s) kp = k;
          if (a.res.vel[k] == s) kv = k;
        }
      } else {
        for (int k = 0; k < U; ++k) {
          if (a.res.pos[k] == s) kp = k;
          if (a.res.vel[k] == s) kv = k;
        }
      }
      kpos[s] = kp;
      kvel[s] = kv;
    }
    if constexpr (PMS) {
      int pv = -1, pp = -1;
      for (int i = 0; i < a.ms.n; ++i) {
        if (a.ms.pos[i] == s) pv = a.ms.vel[i];
        if (a.ms.vel[i] == s) pp = a.ms.pos[i];
      }
      pvel[s] = pv;
      ppos[s] = pp;
    }
  }
  if constexpr (RES) {
    bool sq = tid >= 64 && tid < 64 + U;
    if constexpr (HIST) sq = sq && pdon;
    if (sq) {  // the gains squared once, as the forward squares them
      const int k = tid - 64;
      const double kp = a.res.sqrt_kp[k], kd = a.res.sqrt_kd[k];
      gn2[k] = kp * kp;
      gn2[MCP_MAX_INPUT + k] = kd * kd;
    }
  }
  // a worker thread's entries of the parameter vector: where their delta and their activation sit in a row; the running sums
  const int wt = tid - 128;
  const int nused = (ntot + MB_NWORK - 1) / MB_NWORK;  // (uniform)
  int dof[MB_NACC], aof[MB_NACC];
  double gacc[MB_NACC];
#pragma unroll
  for (int i = 0; i < MB_NACC; ++i) {
    dof[i] = aof[i] = 0;
    gacc[i] = 0.0;
    const int e = wt + MB_NWORK * i;
    if (wt >= 0 && e < ntot) {
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        if (l >= nl) continue;
        if (e >= mg.woff[l] && e < mg.boff[l]) {
          const int j = (e - mg.woff[l]) / mg.in[l];
          dof[i] = L.doff[l] + j;
          aof[i] = L.aoff[l] + (e - mg.woff[l] - j * mg.in[l]);
        } else if (e >= mg.boff[l] && e < mg.boff[l] + mg.out[l]) {
          dof[i] = L.doff[l] + e - mg.boff[l];
          aof[i] = L.one;
        }
      }
      if constexpr (RES) {  // g_sqrt_kp | g_sqrt_kd: delta_out[k] times the row's 2 sqrt_k e
        if (e >= mg.nparam) {
          const int j = e - mg.nparam;
          dof[i] = dlast + (j < U ? j : j - U);
          aof[i] = L.res0 + j;
        }
      }
    }
  }
  const int ww = wv - 2;  // worker wave 0..5

  // the activations of row r of this part's trajectories, worker wave `ww`: a trajectory per wave and turn (from what the forward's network
  // read: the state, in the measured form the measurement)
  auto activations = [&](int r, int mp0) {
    double* ab = act + (r % 3) * pts * L.ap;
    for (int p = ww; p < pts; p += 6) {
      const double* xr = mlp_policy_rows<PMS>(a) + ((size_t)r * M + imin(mp0 + p, M - 1)) * S;
      double* A = ab + p * L.ap;
      if constexpr (HIST) {  // block j from row max(r - j, 0): the forward's statements on the forward's operands
        if (lane < nnp + nap) {
          for (int j = 0; j < nhist; ++j) {
            const double* xj = mlp_policy_rows<PMS>(a) + ((size_t)imax(r - j, 0) * M + imin(mp0 + p, M - 1)) * S;
            if (lane < nnp) {
              A[j * P0 + lane] = xj[pl.non_angle[lane]];
            } else {
              double sn, cs;
              sincos_fast(xj[pl.angle[lane - nnp]], &sn, &cs);
              A[j * P0 + lane] = sn;
              A[j * P0 + lane + nap] = cs;
            }
          }
        }
      } else if (lane < nnp + nap) {
        if (lane < nnp) {
          A[lane] = xr[pl.non_angle[lane]];
        } else {
          double sn, cs;
          sincos_fast(xr[pl.angle[lane - nnp]], &sn, &cs);
          A[lane] = sn;
          A[lane + nap] = cs;
        }
      }
      if constexpr (TRK) {  // the forward's statement on the forward's operands (at most 32 sources: a lane each)
        if (lane >= nnp + nap && lane < nnp + nap + ntr) {
          const int s = a.trk.idx[lane - nnp - nap];
          if constexpr (HIST) {
            A[(nhist - 1) * P0 + lane + nap] = a.trk.target[(size_t)r * S + s] - xr[s];  // (behind the last block)
          } else {
            A[lane + nap] = a.trk.target[(size_t)r * S + s] - xr[s];
          }
        }
      }
      if constexpr (RES) {  // the gain gradients' factors 2 sqrt_k e, e the forward's difference on the forward's operands
        bool gl = lane < 2 * U;
        if constexpr (HIST) gl = gl && pdon;
        if (gl) {
          const bool isp = lane < U;
          const int k = isp ? lane : lane - U;
          const int s = isp ? a.res.pos[k] : a.res.vel[k];
          const double e = a.res.target[(size_t)r * S + s] - xr[s];
          A[L.res0 + lane] = 2.0 * (isp ? a.res.sqrt_kp[k] : a.res.sqrt_kd[k]) * e;
        }
      }
      if (lane == 0) A[L.one] = 1.0;
      wave_lds_sync();
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        if (l + 1 >= nl) continue;  // (uniform)
        if constexpr (DROP) {  // (every lane of the wave is here: the ballot is the layer's row of decisions)
          const bool unit = lane < mg.out[l];
          const bool keep = unit && (alldrop || mlp_keep(nzl, a.drop.thr, Hd, M, imin(mp0 + p, M - 1), r, L.doff[l] + lane));
          const unsigned long long kw = __ballot(keep);
          if (unit) {
            const double h = fast_tanh(mlp_unit(Wl[l] + lane * wp[l], bl[l][lane], A + L.aoff[l], mg.in[l]));
            A[L.aoff[l + 1] + lane] = keep ? a.drop.scale * h : 0.0;
          }
          if (lane == 0) kwl[((r % 3) * pts + p) * 2 + l] = kw;
        } else if (lane < mg.out[l]) {
          A[L.aoff[l + 1] + lane] = fast_tanh(mlp_unit(Wl[l] + lane * wp[l], bl[l][lane], A + L.aoff[l], mg.in[l]));
        }
        wave_lds_sync();
      }
    }
  };
  // this worker thread's entries: the products of row r added over the part's trajectories in order
  auto outer_sums = [&](int r) {
    const double* db = del + (r & 1) * pts * L.dp;
    const double* ab = act + (r % 3) * pts * L.ap;
#pragma unroll
    for (int i = 0; i < MB_NACC; ++i) {
      if (i < nused) {
        for (int p = 0; p < pts; ++p) gacc[i] = fma(db[p * L.dp + dof[i]], ab[p * L.ap + aof[i]], gacc[i]);
      }
    }
  };
  // the loader's work for one row (64 lanes): g_states, the state, the inputs and their upstream gradient of row r; jac[r] where r < T - 1
  auto load_row = [&](int r, int b, int l, int mp0) {
    for (int it = l; it < pts * S; it += 64) {
      const int p = it / S, s = it - p * S;
      if (lenl[p] > 0) {
        gsl[(b * pts + p) * S + s] = a.g_states[((size_t)r * M + mp0 + p) * S + s];
        xsl[(b * pts + p) * S + s] = a.states[((size_t)r * M + mp0 + p) * S + s];
      }
    }
    for (int it = l; it < pts * U; it += 64) {
      const int p = it / U, k = it - p * U;
      if (lenl[p] > 0) {
        ull[(b * pts + p) * U + k] = a.inputs[((size_t)r * M + mp0 + p) * U + k];
        gul[(b * pts + p) * U + k] = a.g_inputs ? a.g_inputs[((size_t)r * M + mp0 + p) * U + k] : 0.0;
      }
    }
    if (r < T - 1)
      for (int it = l; it < pts * GD; it += 64) {
        const int p = it / GD, e = it - p * GD;
        if (lenl[p] > 0) rec[(b * pts + p) * RP + e] = a.jac[((size_t)r * M + mp0 + p) * GD + e];
      }
  };

  for (int part = 0; part * pts < MB_PT; ++part) {
    const int mp0 = blockIdx.x * MB_PT + part * pts;
    if (mp0 >= M) break;  // (uniform) the ragged last tile: nothing of it is left
    if (part > 0) __syncthreads();
    if (tid >= 64 && tid < 64 + pts) lenl[tid - 64] = mp0 + tid - 64 < M ? T : 0;
    for (int it = tid; it < 2 * pts * S; it += MB_NT) lam[it] = 0.0;
    if constexpr (PMS)
      for (int it = tid; it < 2 * pts * S; it += MB_NT) car[it] = 0.0;
    if constexpr (HIST)
      for (int it = tid; it < nhist * pts * S; it += MB_NT) pend[it] = 0.0;
    __syncthreads();
    int b = 0, lc = 0;
    if (wv == 1) load_row(T - 1, 0, lane, mp0);
    if (wv >= 2) activations(T - 1, mp0);
    __syncthreads();
    for (int r = T - 1; r >= 0; --r) {
      if (wv == 1) {
        if (r > 0) load_row(r - 1, b ^ 1, lane, mp0);
      } else if (wv >= 2) {
        if (a.g_params && r + 1 <= T - 1) outer_sums(r + 1);
        if (r > 0) activations(r - 1, mp0);
      } else if ((lane & 15) < pts) {
        const int p = lane & 15, q = lane >> 4;
        const int len = lenl[p];
        const double* lamc = lam + (lc * pts + p) * S;
        double* lamn = lam + ((lc ^ 1) * pts + p) * S;
        const double* rc = rec + (b * pts + p) * RP;
        const double* xc = xsl + (b * pts + p) * S;
        const double* gc = gsl + (b * pts + p) * S;
        const double* Ar = act + ((r % 3) * pts + p) * L.ap;
        double* dr = del + ((r & 1) * pts + p) * L.dp;
        double* fb = fbar + p * L.fp;
        const bool active = r < len - 1;
        // stage A: the adjoints of the increments
        for (int g = q; g < G; g += 4) {
          double acc = 0.0;
          for (int s = 0; s < S; ++s)
            if (ogt[s] == g) acc += post[s] ? 0.5 * a.Ts * lamc[s] : lamc[s];
          gdl[p * G + g] = acc;
        }
        wave_lds_sync();
        // stage B: through the record to the GP input
        if (active) {
          for (int d = q; d < D; d += 4) {
            double acc = 0.0;
            for (int g = 0; g < G; ++g) acc = fma(gdl[p * G + g], rc[g * D + d], acc);
            gzl[p * D + d] = acc;
          }
        }
        wave_lds_sync();
        // stage M: through the squashing and the layers, last to first; the deltas stay in LDS for the workers' outer sums
        for (int k = q; k < U; k += 4) {
          double ab = 0.0;
          if (r <= len - 1) {
            double gu = gul[(b * pts + p) * U + k];
            if (active) gu += gzl[p * D + nna + 2 * na + k];
            ab = gu;
            if (pl.squash) {
              const double th = ull[(b * pts + p) * U + k] / pl.u_max[k];
              ab = gu * (1.0 - th * th);
            }
          }
          dr[dlast + k] = ab;
        }
        wave_lds_sync();
        double acc[MB_CMAX];
#pragma unroll
        for (int l = 2; l >= 1; --l) {  // delta of layer l - 1 from that of layer l
          if (l >= nl) continue;  // (uniform)
          mlp_back(Wl[l], wp[l], mg.in[l], mg.out[l], dr + L.doff[l], q, acc);
#pragma unroll
          for (int i = 0; i < MB_CMAX; ++i) {
            const int j = q + 4 * i;
            if (j < mg.in[l]) {
              const double h = Ar[L.aoff[l] + j];
              if constexpr (DROP) {
                const double th = a.drop.keep_p * h;
                dr[L.doff[l - 1] + j] = (kwl[((r % 3) * pts + p) * 2 + l - 1] >> j & 1ull) ? acc[i] * (a.drop.scale * (1.0 - th * th)) : 0.0;
              } else {
                dr[L.doff[l - 1] + j] = acc[i] * (1.0 - h * h);
              }
            }
          }
          wave_lds_sync();
        }
        mlp_back(Wl[0], wp[0], mg.in[0], mg.out[0], dr + L.doff[0], q, acc);
#pragma unroll
        for (int i = 0; i < MB_CMAX; ++i)
          if (q + 4 * i < mg.in[0]) fb[q + 4 * i] = acc[i];
        wave_lds_sync();
        double* pcur = pend + ((r % nhist) * pts + p) * S;  // (history form) this row's slot of the ring
        (void)pcur;
        if constexpr (HIST) {  // the window's adjoint: the pulls of blocks j >= 1 of this row on the rows max(r - j, 0), j ascending
          if (r <= len - 1)
            for (int s = q; s < S; s += 4)
              for (int j = 1; j < nhist; ++j) {
                double y = 0.0;
                if (fplain[s] >= 0) y += fb[j * P0 + fplain[s]];
                if (fang[s] >= 0)
                  y += fb[j * P0 + nnp + fang[s]] * Ar[j * P0 + nnp + nap + fang[s]] - fb[j * P0 + nnp + nap + fang[s]] * Ar[j * P0 + nnp + fang[s]];
                pend[((imax(r - j, 0) % nhist) * pts + p) * S + s] += y;
              }
          wave_lds_sync();  // row 0 reads below what its own clamped blocks just added
        }
        // stage C: the integrator and the two feature maps
        for (int s = q; s < S; s += 4) {
          double v = 0.0;
          if (r == len - 1) {
            v = gc[s];
          } else if (active) {
            v = gc[s];
            if (ogt[s] >= 0) v += lamc[s];
            for (int s2 = 0; s2 < S; ++s2)
              if (velof[s2] == s) v = fma(a.Ts, lamc[s2], v);
            if (zplain[s] >= 0) v += gzl[p * D + zplain[s]];
            if (zang[s] >= 0) {
              double sn, cs;
              sincos_fast(xc[s], &sn, &cs);
              v += gzl[p * D + nna + zang[s]] * cs - gzl[p * D + nna + na + zang[s]] * sn;
            }
          }
          if constexpr (!PMS) {
            if (r <= len - 1) {
              if (fplain[s] >= 0) v += fb[fplain[s]];
              if (fang[s] >= 0) v += fb[nnp + fang[s]] * Ar[nnp + nap + fang[s]] - fb[nnp + nap + fang[s]] * Ar[nnp + fang[s]];
              if constexpr (TRK) {
                if constexpr (HIST) {
                  if (ferr[s] >= 0) v -= fb[nhist * P0 + ferr[s]];  // (behind the last block)
                } else {
                  if (ferr[s] >= 0) v -= fb[nnp + 2 * nap + ferr[s]];  // e = target - x
                }
              }
              if constexpr (RES) {
                if (kpos[s] >= 0) v -= gn2[kpos[s]] * dr[dlast + kpos[s]];
                if (kvel[s] >= 0) v -= gn2[MCP_MAX_INPUT + kvel[s]] * dr[dlast + kvel[s]];
              }
              if constexpr (HIST) v += pcur[s];
            }
          } else if (r <= len - 1) {
            auto ybar = [&](int c) {  // the policy's pull on component c of the measurement
              double y = 0.0;
              if (fplain[c] >= 0) y += fb[fplain[c]];
              if (fang[c] >= 0) y += fb[nnp + fang[c]] * Ar[nnp + nap + fang[c]] - fb[nnp + nap + fang[c]] * Ar[nnp + fang[c]];
              if constexpr (TRK) {
                if (ferr[c] >= 0) y -= fb[nnp + 2 * nap + ferr[c]];  // e = target - y
              }
              if constexpr (RES) {
                if (kpos[c] >= 0) y -= gn2[kpos[c]] * dr[dlast + kpos[c]];
                if (kvel[c] >= 0) y -= gn2[MCP_MAX_INPUT + kvel[c]] * dr[dlast + kvel[c]];
              }
              return y;
            };
            const int pv = pvel[s], pp = ppos[s];
            if (pv >= 0) {  // a measured position: the filter's adjoint of its pair
              double* cr = car + (p * S + s) * 2;
              const double mvn = cr[0], nvn = cr[1];
              if (r >= 1) {
                const double mvb = ybar(pv) - (a.ms.a1 / a.ms.a0) * mvn;
                const double nvb = (a.ms.b0 / a.ms.a0) * mvb + (a.ms.b1 / a.ms.a0) * mvn;
                v += ybar(s) + (nvb - nvn) / a.Ts;
                cr[0] = mvb;
                cr[1] = nvb;
              } else {
                v += ybar(s) - nvn / a.Ts;
              }
            } else if (pp >= 0) {  // a measured velocity: seen true in row 0 only, where it also started both histories
              if (r == 0) v += ybar(s) + ((a.ms.b1 - a.ms.a1) / a.ms.a0) * car[(p * S + pp) * 2];
            } else {
              v += ybar(s);
            }
          }
          lamn[s] = v;
        }
        wave_lds_sync();
        if constexpr (HIST) {  // behind the slot's reader: it now serves row r - hist
          for (int s = q; s < S; s += 4) pcur[s] = 0.0;
          wave_lds_sync();
        }
        lc ^= 1;
      }
      __syncthreads();
      b ^= 1;
    }
    // (T is the same for every lane: the chain wave flipped lc T times)
    lc = T & 1;
    if (wv >= 2 && a.g_params) outer_sums(0);
    if (wv == 0 && a.g_x0) {
      const int p = lane & 15, q = lane >> 4;
      if (p < pts && lenl[p] > 0)
        for (int s = q; s < S; s += 4) a.g_x0[(size_t)(mp0 + p) * S + s] = lam[(lc * pts + p) * S + s];
    }
  }
  if (wt >= 0 && a.g_params) {
#pragma unroll
    for (int i = 0; i < MB_NACC; ++i) {
      const int e = wt + MB_NWORK * i;
      if (e < ntot) a.g_params[(size_t)blockIdx.x * ntot + e] = gacc[i];
    }
  }
}

// what mcp_rollout_mlp_bwd, mcp_rollout_mlp_meas_bwd and mcp_rollout_mlp_drop_bwd share (ms NULL: no measurement; p_drop 0: the kernels
// without dropout, and `noise` is not looked at)
template <bool WLDS, bool PMS, bool DROP = false, bool TRK = false, bool RES = false, bool HIST = false>
static int launch_mlp_bwd(const typename MlpBwdKernelArgs<PMS, DROP, TRK, RES, HIST>::type& a, size_t lds, hipStream_t st) {
  MCP_ENSURE_MAX_LDS((rollout_mlp_bwd_kernel<WLDS, PMS, DROP, TRK, RES, HIST>));
  hipLaunchKernelGGL((rollout_mlp_bwd_kernel<WLDS, PMS, DROP, TRK, RES, HIST>), dim3((a.M + MB_PT - 1) / MB_PT), dim3(MB_NT), lds, st, a);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}
template <bool PMS, class Args>
static int launch_mlp_bwd_drop(const Args& a, const mcp_noise* noise, double p_drop, size_t lds, hipStream_t st) {
  MlpBwdArgsDrop<PMS> d = mlp_with_drop<MlpBwdArgsDrop<PMS>, Args>(a, p_drop);
  d.nz = *noise;
  return a.wlds ? launch_mlp_bwd<true, PMS, true>(d, lds, st) : launch_mlp_bwd<false, PMS, true>(d, lds, st);
}
// a tracking sweep: the dropout form's arguments at any p_drop (the noise only where decisions are drawn again), and the track
template <bool PMS, class Args>
static int launch_mlp_bwd_track(const Args& a, const mcp_noise* noise, double p_drop, const mcp_mlp_track* trk, size_t lds, hipStream_t st) {
  MlpBwdArgsTrack<PMS> d = mlp_with_track<MlpBwdArgsTrack<PMS>, Args>(a, p_drop, trk);
  memset(&d.nz, 0, sizeof(d.nz));
  if (noise && p_drop > 0.0) d.nz = *noise;
  return a.wlds ? launch_mlp_bwd<true, PMS, true, true>(d, lds, st) : launch_mlp_bwd<false, PMS, true, true>(d, lds, st);
}
// a residual sweep: the tracking form's arguments (with or without errors), and the PD term
template <bool PMS, class Args>
static int launch_mlp_bwd_res(const Args& a, const mcp_noise* noise, double p_drop, const mcp_mlp_track* trk, const mcp_mlp_pd* res, size_t lds,
                              hipStream_t st) {
  MlpBwdArgsRes<PMS> d = mlp_with_res<MlpBwdArgsRes<PMS>, Args>(a, p_drop, trk, res);
  memset(&d.nz, 0, sizeof(d.nz));
  if (noise && p_drop > 0.0) d.nz = *noise;
  return a.wlds ? launch_mlp_bwd<true, PMS, true, true, true>(d, lds, st) : launch_mlp_bwd<false, PMS, true, true, true>(d, lds, st);
}
// a history sweep: the residual form's arguments (with or without the PD term), and the depth of the window
static int launch_mlp_bwd_hist(const MlpBwdArgs& a, const mcp_noise* noise, double p_drop, const mcp_mlp_track* trk, const mcp_mlp_pd* res,
                               const mcp_mlp_hist* hs, size_t lds, hipStream_t st) {
  MlpBwdArgsHist<false> d = mlp_with_hist<MlpBwdArgsHist<false>, MlpBwdArgs>(a, p_drop, trk, res, hs);
  memset(&d.nz, 0, sizeof(d.nz));
  if (noise && p_drop > 0.0) d.nz = *noise;
  return a.wlds ? launch_mlp_bwd<true, false, true, true, true, true>(d, lds, st) : launch_mlp_bwd<false, false, true, true, true, true>(d, lds, st);
}

// The history forms are instantiated in a translation unit of their own (rollout_mlp_hist.hip): they are a fifth of this family's kernels, and
// the family's kernels are the library's longest compile.  What rollout_mlp.hip's two dispatchers call there, after their checks and fills
// (``a``: the filled arguments; the history forms are instantiated WITHOUT a measurement model -- the entries refuse the pair):
namespace mcp {
int launch_mlp_hist(const OpenArgsMlpMeas& a, double p_drop, const mcp_mlp_track* trk, const mcp_mlp_pd* res, const mcp_mlp_hist* hist, int maxdeg,
                    bool wantvar, hipStream_t st);
int launch_mlp_hist_bwd(const MlpBwdArgsMeas& a, const mcp_noise* noise, double p_drop, const mcp_mlp_track* trk, const mcp_mlp_pd* res,
                        const mcp_mlp_hist* hist, size_t lds, hipStream_t st);
}  // namespace mcp
