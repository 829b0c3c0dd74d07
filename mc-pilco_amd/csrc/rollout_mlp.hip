// Fused closed loop under a tanh multilayer perceptron for gfx950 (MI355X), and its reverse-time sweep: the host dispatch and the C entries
// mcp_rollout_mlp* / mcp_rollout_mlp*_bwd.  The kernels, their layouts and the account of the family are in rollout_mlp_kernels.h; this
// translation unit instantiates every form of them but the history forms (rollout_mlp_hist.hip).
#include "rollout_mlp_kernels.h"

// what mcp_rollout_mlp, mcp_rollout_mlp_meas, mcp_rollout_mlp_drop, mcp_rollout_mlp_track and mcp_rollout_mlp_res share (ms NULL: no
// measurement; p_drop 0: the kernels without dropout; trk NULL or n == 0: the kernels without the error features; res NULL or on == 0:
// the kernels without the PD term)
static int mlp_dispatch(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* ms, const mcp_noise* noise, double p_drop, int M, int T,
                        int particle_pred, const double* x0, double* states, double* inputs, double* mu, double* var, double* jac,
                        uint32_t* status, void* stream, const mcp_mlp_track* trk = nullptr, const mcp_mlp_pd* res = nullptr,
                        const mcp_mlp_hist* hist = nullptr) {
  const int crc = closed_loop_checks(model && mlp && noise && x0 && states && inputs && status && mlp_drop_ok(p_drop), M, T, model, ms, false, [&] {
    const int prc = mlp_policy_check(model, mlp, trk, T, hist);
    return prc != MCP_OK ? prc : mlp_res_check(mlp, res, T);
  });
  if (crc != MCP_OK) return crc;
  if (hist_active(hist) && meas_active(ms)) return MCP_ERR_ARG;  // (the history forms have no measured form: DESIGN section 7)
  OpenArgsMlpMeas a;
  // (T == 1: the policy alone -- no transition, nothing to record)
  const int maxdeg = open_fill(a, model, noise, M, T, particle_pred, x0, nullptr, M, nullptr, states, mu, var, T == 1 ? nullptr : jac, status);
  a.mlp = mlp_normalised(mlp);
  a.inputs = inputs;
  hipStream_t st = (hipStream_t)stream;
  if (hist_active(hist))  // (with or without the errors, the PD term, dropout: rollout_mlp_hist.hip)
    return launch_mlp_hist(a, p_drop, trk, res, hist, maxdeg, var != nullptr, st);
  if (res_active(res)) {
    if (!meas_active(ms))
      return launch_mlp_tiles<false, true, true, true>(mlp_with_res<OpenArgsMlpRes<false>, OpenArgsMlp>(a, p_drop, trk, res), maxdeg, var != nullptr, st);
    a.ms = *ms;
    return launch_mlp_tiles<true, true, true, true>(mlp_with_res<OpenArgsMlpRes<true>, OpenArgsMlpMeas>(a, p_drop, trk, res), maxdeg, var != nullptr, st);
  }
  if (track_active(trk)) {
    if (!meas_active(ms))
      return launch_mlp_tiles<false, true, true>(mlp_with_track<OpenArgsMlpTrack<false>, OpenArgsMlp>(a, p_drop, trk), maxdeg, var != nullptr, st);
    a.ms = *ms;
    return launch_mlp_tiles<true, true, true>(mlp_with_track<OpenArgsMlpTrack<true>, OpenArgsMlpMeas>(a, p_drop, trk), maxdeg, var != nullptr, st);
  }
  const bool drop = p_drop > 0.0;
  if (!meas_active(ms)) {
    if (drop) return launch_mlp_tiles<false, true>(mlp_with_drop<OpenArgsMlpDrop<false>, OpenArgsMlp>(a, p_drop), maxdeg, var != nullptr, st);
    return launch_mlp_tiles<false>(a, maxdeg, var != nullptr, st);  // (the base part of `a`: mcp_rollout_mlp's own kernels)
  }
  a.ms = *ms;
  if (drop) return launch_mlp_tiles<true, true>(mlp_with_drop<OpenArgsMlpDrop<true>, OpenArgsMlpMeas>(a, p_drop), maxdeg, var != nullptr, st);
  return launch_mlp_tiles<true>(a, maxdeg, var != nullptr, st);
}

extern "C" int mcp_rollout_mlp(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_noise* noise, int M, int T, int particle_pred,
                               const double* x0, double* states, double* inputs, double* mu, double* var, double* jac, uint32_t* status,
                               void* stream) {
  return mlp_dispatch(model, mlp, nullptr, noise, 0.0, M, T, particle_pred, x0, states, inputs, mu, var, jac, status, stream);
}

// Closed-loop rollout under the network evaluated on a simulated measurement: replaces the loop of MC_PILCO4PMS.apply_policy
// (policy_learning/MC_PILCO.py:808-906: noisy positions, backward-difference velocities, the first-order filter) with Policy.MLP_policy as
// the policy, over Model_learning.get_next_state (model_learning/Model_learning.py:210-229, 471-494, 685-718).  meas->n == 0:
// mcp_rollout_mlp's kernels on the same arguments.
extern "C" int mcp_rollout_mlp_meas(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* meas, const mcp_noise* noise, int M, int T,
                                    int particle_pred, const double* x0, double* states, double* inputs, double* mu, double* var, double* jac,
                                    uint32_t* status, void* stream) {
  if (!meas) return MCP_ERR_ARG;
  return mlp_dispatch(model, mlp, meas, noise, 0.0, M, T, particle_pred, x0, states, inputs, mu, var, jac, status, stream);
}

// mcp_rollout_mlp / mcp_rollout_mlp_meas with inverted dropout on the hidden units (MC-PILCO's regulariser, as policy_learning/Policy.py:223-225, 261
// has it for the RBF policies' basis functions): the DROP forms of rollout_mlp_kernels.h.  meas NULL or meas->n == 0: the network sees the true state.  p_drop == 0: the kernels of the
// entries without dropout on the same arguments, the same bits.
extern "C" int mcp_rollout_mlp_drop(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* meas, const mcp_noise* noise, double p_drop,
                                    int M, int T, int particle_pred, const double* x0, double* states, double* inputs, double* mu, double* var,
                                    double* jac, uint32_t* status, void* stream) {
  return mlp_dispatch(model, mlp, meas, noise, p_drop, M, T, particle_pred, x0, states, inputs, mu, var, jac, status, stream);
}

// mcp_rollout_mlp_drop with the target-trajectory features of the reference's Sum_of_gaussians_with_target_trajectory (policy_in =
// cat(x, x*_t - x), policy_learning/Policy.py:389-403) behind the network's own: the TRK forms of rollout_mlp_kernels.h, over the loops the other entries
// replace (policy_learning/MC_PILCO.py:615-674, measured :808-906).  track NULL or track->n == 0: the kernels of mcp_rollout_mlp_drop on the
// same arguments, the same bits.
extern "C" int mcp_rollout_mlp_track(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_track* track, const mcp_meas* meas,
                                     const mcp_noise* noise, double p_drop, int M, int T, int particle_pred, const double* x0, double* states,
                                     double* inputs, double* mu, double* var, double* jac, uint32_t* status, void* stream) {
  return mlp_dispatch(model, mlp, meas, noise, p_drop, M, T, particle_pred, x0, states, inputs, mu, var, jac, status, stream, track);
}

// mcp_rollout_mlp_track with the PD term of the residual policy, u = squash(PD(x, t) + net(x, t)) -- the UR5 launch script's tracking
// controller (PD_controller.forward, policy_learning/Policy.py:406-449) kept, and Policy.MLP_policy as its correction under the one
// squashing: the RES forms of rollout_mlp_kernels.h, over the loops the other entries replace (policy_learning/MC_PILCO.py:615-674, measured :808-906).
// res NULL or res->on == 0: the kernels of mcp_rollout_mlp_track on the same arguments, the same bits.
extern "C" int mcp_rollout_mlp_res(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_track* track, const mcp_mlp_pd* res,
                                   const mcp_meas* meas, const mcp_noise* noise, double p_drop, int M, int T, int particle_pred, const double* x0,
                                   double* states, double* inputs, double* mu, double* var, double* jac, uint32_t* status, void* stream) {
  return mlp_dispatch(model, mlp, meas, noise, p_drop, M, T, particle_pred, x0, states, inputs, mu, var, jac, status, stream, track, res);
}

// mcp_rollout_mlp_res with a window of the last hist->h rows in front of layer 0: the network with memory (template HIST of rollout_mlp_kernels.h,
// instantiated in rollout_mlp_hist.hip), over the
// loop of MC_PILCO.apply_policy (policy_learning/MC_PILCO.py:615-674); hist->h > 1 with an active measurement model: MCP_ERR_ARG (no measured
// form is built).  hist NULL or hist->h == 1: the kernels of
// mcp_rollout_mlp_res on the same arguments, the same bits.
extern "C" int mcp_rollout_mlp_hist(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_hist* hist, const mcp_mlp_track* track,
                                    const mcp_mlp_pd* res, const mcp_meas* meas, const mcp_noise* noise, double p_drop, int M, int T,
                                    int particle_pred, const double* x0, double* states, double* inputs, double* mu, double* var, double* jac,
                                    uint32_t* status, void* stream) {
  return mlp_dispatch(model, mlp, meas, noise, p_drop, M, T, particle_pred, x0, states, inputs, mu, var, jac, status, stream, track, res, hist);
}

static int mlp_bwd_dispatch(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* ms, const mcp_noise* noise, double p_drop, int M, int T,
                            const double* states, const double* inputs, const double* jac, const double* g_states, const double* g_inputs,
                            double* g_params, double* g_x0, void* stream, const mcp_mlp_track* trk = nullptr, const mcp_mlp_pd* res = nullptr,
                            const mcp_mlp_hist* hist = nullptr) {
  const bool hst = hist_active(hist);  // (a history form is a residual form, whatever of the track and the PD term is on)
  const bool drop = p_drop > 0.0, resid = res_active(res) || hst, track = track_active(trk) || resid;
  const int crc = closed_loop_checks(model && mlp && states && inputs && g_states && (jac || T <= 1) && mlp_drop_ok(p_drop) && (noise || !drop), M, T,
                                     model, ms, true, [&] {
                                       const int prc = mlp_policy_check(model, mlp, trk, T, hist);
                                       return prc != MCP_OK ? prc : mlp_res_check(mlp, res, T);
                                     });
  if (crc != MCP_OK) return crc;
  if (hist_active(hist) && meas_active(ms)) return MCP_ERR_ARG;  // (the history forms have no measured form)
  if (!g_x0 && !g_params) return MCP_OK;  // nothing asked for
  const bool pms = meas_active(ms);
  MlpBwdArgsMeas a;
  memset(&a, 0, sizeof(a));
  sweep_fill_model(a, model, M, T);
  a.states = states, a.inputs = inputs, a.jac = jac, a.g_states = g_states, a.g_inputs = g_inputs, a.g_x0 = g_x0, a.g_params = g_params;
  a.mlp = mlp_normalised(mlp);
  if (pms) a.ms = *ms;
  // the part of the tile swept at once: the largest whose layout fits, the weights in LDS where they then fit too
  const MlpGeom mg = mlp_geom(a.mlp);
  size_t lds = 0;
  for (int pts = MB_PT; pts >= 1 && !a.pts; pts >>= 1)
    for (int wl = 1; wl >= 0 && !a.pts; --wl) {
      const MlpBwdLayout L = mlp_bwd_layout(pts, a.S, a.U, a.G, a.D, a.mlp, mg, wl != 0, pms, drop || track, track, resid, hst ? hist->h : 1);
      lds = (size_t)L.total * sizeof(double);
      if (lds <= MCP_LDS_LIMIT) a.pts = pts, a.wlds = wl;
    }
  if (!a.pts) return MCP_ERR_LIMIT;  // (not reached within the compiled limits: one trajectory takes 22 KB at all of them at once)
  hipStream_t st = (hipStream_t)stream;
  if (hst) return launch_mlp_hist_bwd(a, noise, p_drop, trk, res, hist, lds, st);  // (rollout_mlp_hist.hip)
  if (resid)
    return pms ? launch_mlp_bwd_res<true, MlpBwdArgsMeas>(a, noise, p_drop, trk, res, lds, st)
               : launch_mlp_bwd_res<false, MlpBwdArgs>(a, noise, p_drop, trk, res, lds, st);
  if (track)
    return pms ? launch_mlp_bwd_track<true, MlpBwdArgsMeas>(a, noise, p_drop, trk, lds, st) : launch_mlp_bwd_track<false, MlpBwdArgs>(a, noise, p_drop, trk, lds, st);
  if (drop) return pms ? launch_mlp_bwd_drop<true, MlpBwdArgsMeas>(a, noise, p_drop, lds, st) : launch_mlp_bwd_drop<false, MlpBwdArgs>(a, noise, p_drop, lds, st);
  if (pms) return a.wlds ? launch_mlp_bwd<true, true>(a, lds, st) : launch_mlp_bwd<false, true>(a, lds, st);
  return a.wlds ? launch_mlp_bwd<true, false>(a, lds, st) : launch_mlp_bwd<false, false>(a, lds, st);  // (the base part of `a`: mcp_rollout_mlp_bwd's own kernels)
}

extern "C" int mcp_rollout_mlp_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, int M, int T, const double* states, const double* inputs,
                                   const double* jac, const double* g_states, const double* g_inputs, double* g_params, double* g_x0,
                                   void* stream) {
  return mlp_bwd_dispatch(model, mlp, nullptr, nullptr, 0.0, M, T, states, inputs, jac, g_states, g_inputs, g_params, g_x0, stream);
}

// Reverse-time sweep of the closed loop under the network on the simulated measurement: replaces autograd's backward (MC_PILCO.py:522)
// through the loop of MC_PILCO4PMS.apply_policy (policy_learning/MC_PILCO.py:808-906, the filter recursion included), Policy.MLP_policy and
// get_next_state with its integrators (model_learning/Model_learning.py:210-229, 471-494, 685-718), from the record and meas->meas alone.
// meas->n == 0: mcp_rollout_mlp_bwd's kernels.
extern "C" int mcp_rollout_mlp_meas_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* meas, int M, int T, const double* states,
                                        const double* inputs, const double* jac, const double* g_states, const double* g_inputs, double* g_params,
                                        double* g_x0, void* stream) {
  if (!meas) return MCP_ERR_ARG;
  return mlp_bwd_dispatch(model, mlp, meas, nullptr, 0.0, M, T, states, inputs, jac, g_states, g_inputs, g_params, g_x0, stream);
}

// Reverse-time sweep of mcp_rollout_mlp_drop: the keep decisions are the forward's, recomputed from the same noise descriptor (the mask
// buffer, or seed / call / particle_offset / call_dev), which is required when p_drop > 0.  p_drop == 0: the kernels of the sweeps without
// dropout, the same bits.
extern "C" int mcp_rollout_mlp_drop_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_meas* meas, const mcp_noise* noise, double p_drop,
                                        int M, int T, const double* states, const double* inputs, const double* jac, const double* g_states,
                                        const double* g_inputs, double* g_params, double* g_x0, void* stream) {
  return mlp_bwd_dispatch(model, mlp, meas, noise, p_drop, M, T, states, inputs, jac, g_states, g_inputs, g_params, g_x0, stream);
}

// Reverse-time sweep of mcp_rollout_mlp_track: the TRK forms of the sweep in rollout_mlp_kernels.h -- the error features recomputed in the activation rows,
// their pull lambda[idx[i]] -= fbar[n_non_angle + 2 n_angle + i] in stage C (measured form: in the pull on the measurement).  track NULL or
// track->n == 0: the kernels of mcp_rollout_mlp_drop_bwd on the same arguments, the same bits.
extern "C" int mcp_rollout_mlp_track_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_track* track, const mcp_meas* meas,
                                         const mcp_noise* noise, double p_drop, int M, int T, const double* states, const double* inputs,
                                         const double* jac, const double* g_states, const double* g_inputs, double* g_params, double* g_x0,
                                         void* stream) {
  return mlp_bwd_dispatch(model, mlp, meas, noise, p_drop, M, T, states, inputs, jac, g_states, g_inputs, g_params, g_x0, stream, track);
}

// Reverse-time sweep of mcp_rollout_mlp_res: the RES forms of the sweep in rollout_mlp_kernels.h -- the PD term's pull on the state in stage C (measured form:
// on the measurement), the gain gradients g_sqrt_kp [U] | g_sqrt_kd [U] behind bout in every slab of n_param + 2 U entries.  res NULL or
// res->on == 0: the kernels of mcp_rollout_mlp_track_bwd on the same arguments, the same bits.  Replaces autograd's backward
// (MC_PILCO.py:522) through the loops named at the forward entry.
extern "C" int mcp_rollout_mlp_res_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_track* track, const mcp_mlp_pd* res,
                                       const mcp_meas* meas, const mcp_noise* noise, double p_drop, int M, int T, const double* states,
                                       const double* inputs, const double* jac, const double* g_states, const double* g_inputs, double* g_params,
                                       double* g_x0, void* stream) {
  return mlp_bwd_dispatch(model, mlp, meas, noise, p_drop, M, T, states, inputs, jac, g_states, g_inputs, g_params, g_x0, stream, track, res);
}

// Reverse-time sweep of mcp_rollout_mlp_hist: the HIST forms of the sweep in rollout_mlp_kernels.h -- the window recomputed in the activation rows, the pulls
// of its older blocks carried down the rows in a ring of hist slots per trajectory and state component.  hist NULL or hist->h == 1: the
// kernels of mcp_rollout_mlp_res_bwd on the same arguments, the same bits.  Replaces autograd's backward (MC_PILCO.py:522) through the
// loops named at the forward entry.
extern "C" int mcp_rollout_mlp_hist_bwd(const mcp_model* model, const mcp_mlp_policy* mlp, const mcp_mlp_hist* hist, const mcp_mlp_track* track,
                                        const mcp_mlp_pd* res, const mcp_meas* meas, const mcp_noise* noise, double p_drop, int M, int T,
                                        const double* states, const double* inputs, const double* jac, const double* g_states,
                                        const double* g_inputs, double* g_params, double* g_x0, void* stream) {
  return mlp_bwd_dispatch(model, mlp, meas, noise, p_drop, M, T, states, inputs, jac, g_states, g_inputs, g_params, g_x0, stream, track, res, hist);
}
