// Expected-cost kernels for gfx950: Expected_cost.forward (policy_learning/Cost_function.py:25-36)
// with cart_pole_cost (:170-182), saturated_distance_from_trajectory (:124-147) or the target-state
// costs distance_from_target / saturated_distance_from_target (:53-101), and their state gradient.
// HBM-bound elementwise + per-time-step reductions over the particle axis.
// The target-state distance is summed in the difference form sum_i ((x_i - x*_i) / l_i)^2; the reference
// expands it (||x/l||^2 + ||x*/l||^2 - 2 (x/l).(x*/l)), which only adds cancellation: the two agree to the
// rounding of the expanded form, within the 1e-12 the reference's fixture is held to.
// cost_u_fwd_kernel / cost_u_bwd_kernel add control-effort and input-rate terms on the applied inputs (mcp_cost_inputs; no counterpart in the
// reference) and the gradient in the inputs; the five kernels of the state costs are untouched by them.
// cost_rows_kernel / cost_rows_sums_kernel / cost_*bwd_shaped_kernel evaluate the time-weighted, risk-sensitive objective (mcp_objective; no
// counterpart in the reference either) on the costs and moments the forward kernels leave; every kernel above is untouched by them.
#include "cost_point.h"  // cost_point, input_dist, cost_u_point; cost_ok, cost_inputs_ok, cost_inputs_none

// one workgroup per time step: costs[t][:], then mean and centred sum of squares (two passes,
// like torch.mean / torch.std)
__global__ __launch_bounds__(256) void cost_fwd_kernel(mcp_cost c, int T, int M, const double* __restrict__ states,
                                                       double* __restrict__ costs, double* __restrict__ moments,
                                                       uint32_t* __restrict__ status) {
  __shared__ double red[4];
  __shared__ double mean_s;
  const int t = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  double s = 0.0;
  uint32_t bad = 0;
  for (int m = tid; m < M; m += 256) {
    double v = cost_point(c, states + ((size_t)t * M + m) * c.S, t, nullptr);
    costs[(size_t)t * M + m] = v;
    if (is_bad(v)) bad |= MCP_STATUS_NAN;
    s += v;
  }
  s = wave_sum(s);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  if (tid == 0) mean_s = ((red[0] + red[1]) + (red[2] + red[3])) / (double)M;
  __syncthreads();
  const double mean = mean_s;
  double q = 0.0;
  for (int m = tid; m < M; m += 256) {
    double d = costs[(size_t)t * M + m] - mean;
    q = fma(d, d, q);
  }
  q = wave_sum(q);
  __syncthreads();
  if (lane == 0) red[wv] = q;
  __syncthreads();
  if (tid == 0) {
    moments[2 * t] = mean;
    moments[2 * t + 1] = (red[0] + red[1]) + (red[2] + red[3]);
  }
  if (bad) atomicOr(status, bad);
}

// pooled mean / unbiased std over R ranks (Chan et al. parallel-variance combine), then the sums
// over time.  One workgroup.
struct RankCounts {
  int64_t n[64];
};
__global__ __launch_bounds__(256) void cost_finalize_kernel(int T, int R, const double* __restrict__ moments, RankCounts rc,
                                                            double* __restrict__ out) {
  const int64_t* counts = rc.n;
  __shared__ double red[2][4];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  double n_tot = 0.0;
  for (int r = 0; r < R; ++r) n_tot += (double)counts[r];
  double cs = 0.0, ss = 0.0;
  for (int t = tid; t < T; t += 256) {
    double mean = 0.0;
    for (int r = 0; r < R; ++r) mean += (double)counts[r] * moments[((size_t)r * T + t) * 2];
    mean /= n_tot;
    double m2 = 0.0;
    for (int r = 0; r < R; ++r) {
      double d = moments[((size_t)r * T + t) * 2] - mean;
      m2 += moments[((size_t)r * T + t) * 2 + 1] + (double)counts[r] * d * d;
    }
    cs += mean;
    ss += sqrt(m2 / (n_tot - 1.0));
  }
  cs = wave_sum(cs);
  ss = wave_sum(ss);
  if (lane == 0) {
    red[0][wv] = cs;
    red[1][wv] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// Summable form of one rank's moments, for the single all-reduce of a particle-sharded step:
//   sums[t] = sum_m (c - shift_t),  sums[T + t] = sum_m (c - shift_t)^2   over this rank's M particles,
// from the two-pass {mean, centred sum of squares} cost_fwd_kernel produced.  shift (same on every rank; NULL = 0) keeps
// the pooled variance free of cancellation: the caller passes the previous step's pooled means.
__global__ void cost_sums_kernel(int T, double n, const double* __restrict__ moments, const double* __restrict__ shift,
                                 double* __restrict__ sums) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const double d = moments[2 * t] - (shift ? shift[t] : 0.0);
  sums[t] = n * d;
  sums[T + t] = fma(n * d, d, moments[2 * t + 1]);
}

// all ranks' sums added up (n_total particles) -> out[0] = sum_t mean, out[1] = sum_t unbiased std; mean_out[t] (optional)
// receives the pooled mean per time step (the next step's shift).  One workgroup.
__global__ __launch_bounds__(256) void cost_finalize_sums_kernel(int T, double n_tot, const double* __restrict__ sums,
                                                                 const double* __restrict__ shift, double* __restrict__ out,
                                                                 double* __restrict__ mean_out) {
  __shared__ double red[2][4];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  double cs = 0.0, ss = 0.0;
  for (int t = tid; t < T; t += 256) {
    const double a = sums[t], b = sums[T + t];
    const double mean = (shift ? shift[t] : 0.0) + a / n_tot;
    const double m2 = b - a * a / n_tot;
    cs += mean;
    ss += sqrt(fmax(m2, 0.0) / (n_tot - 1.0));
    if (mean_out) mean_out[t] = mean;
  }
  cs = wave_sum(cs);
  ss = wave_sum(ss);
  if (lane == 0) {
    red[0][wv] = cs;
    red[1][wv] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

__global__ void cost_bwd_kernel(mcp_cost c, int T, int M, const double* __restrict__ states, const double* __restrict__ g_cost,
                                double gscale, double* __restrict__ g_states) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)T * M) return;
  int t = (int)(i / M);
  const double* x = states + i * c.S;
  double* g = g_states + i * c.S;
  double dist;
  cost_point(c, x, t, &dist);
  double e = (g_cost ? *g_cost : 1.0) * gscale;
  if (c.kind != MCP_COST_TARGET_QUAD) e *= exp(-dist);  // d c / d dist = exp(-dist); 1 for the plain distance
  for (int s = 0; s < c.S; ++s) g[s] = 0.0;
  if (c.kind == MCP_COST_CARTPOLE) {
    double th = x[c.angle_index];
    double a = (fabs(th) - c.target_angle) / c.ls_angle;
    double b = (x[c.pos_index] - c.target_pos) / c.ls_pos;
    double sg = th > 0.0 ? 1.0 : (th < 0.0 ? -1.0 : 0.0);  // d|theta|/dtheta, 0 at 0 like torch.abs
    g[c.angle_index] += e * 2.0 * a * sg / c.ls_angle;
    g[c.pos_index] += e * 2.0 * b / c.ls_pos;
  } else if (c.kind == MCP_COST_TRAJ) {
    for (int k = 0; k < c.n_used; ++k) {
      int s = c.used[k];
      double r = (x[s] - c.target_traj[(size_t)t * c.S + s]) / c.lengthscales[k];
      g[s] += e * 2.0 * r / c.lengthscales[k];
    }
  } else {  // (an index listed twice accumulates, as torch's indexing backward does)
    for (int k = 0; k < c.n_used; ++k) {
      int s = c.used[k];
      double r = (x[s] - c.target_traj[k]) / c.lengthscales[k];
      g[s] += e * 2.0 * r / c.lengthscales[k];
    }
  }
}

// The factor a on the input terms of one (t, m) and (b_out) the factor b on d d_x / dx, G = g_cost gscale:
// ADD: a = G, b = G f'(d_x);  JOINT: a = b = G f'(d_x + d_u + d_r).
__device__ __forceinline__ double cost_u_factors(const mcp_cost& c, const mcp_cost_inputs& ci, const double* x, const double* u,
                                                 const double* up, int t, double G, double* b_out) {
  const bool quad = c.kind == MCP_COST_TARGET_QUAD;
  double dx;
  cost_point(c, x, t, &dx);
  if (ci.mode == MCP_COST_U_ADD) {
    if (b_out) *b_out = quad ? G : G * exp(-dx);
    return G;
  }
  double du, dr;
  input_dist(ci, u, up, &du, &dr);
  const double a = quad ? G : G * exp(-((dx + du) + dr));
  if (b_out) *b_out = a;
  return a;
}

// cost_fwd_kernel with the input terms: one workgroup per time step, the same two passes and reduction order
__global__ __launch_bounds__(256) void cost_u_fwd_kernel(mcp_cost c, mcp_cost_inputs ci, int T, int M, const double* __restrict__ states,
                                                         const double* __restrict__ inputs, double* __restrict__ costs,
                                                         double* __restrict__ moments, uint32_t* __restrict__ status) {
  __shared__ double red[4];
  __shared__ double mean_s;
  const int t = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  double s = 0.0;
  uint32_t bad = 0;
  for (int m = tid; m < M; m += 256) {
    const size_t i = (size_t)t * M + m;
    const double* u = inputs + i * ci.U;
    double v = cost_u_point(c, ci, states + i * c.S, u, t > 0 ? u - (size_t)M * ci.U : nullptr, t);
    costs[i] = v;
    if (is_bad(v)) bad |= MCP_STATUS_NAN;
    s += v;
  }
  s = wave_sum(s);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  if (tid == 0) mean_s = ((red[0] + red[1]) + (red[2] + red[3])) / (double)M;
  __syncthreads();
  const double mean = mean_s;
  double q = 0.0;
  for (int m = tid; m < M; m += 256) {
    double d = costs[(size_t)t * M + m] - mean;
    q = fma(d, d, q);
  }
  q = wave_sum(q);
  __syncthreads();
  if (lane == 0) red[wv] = q;
  __syncthreads();
  if (tid == 0) {
    moments[2 * t] = mean;
    moments[2 * t + 1] = (red[0] + red[1]) + (red[2] + red[3]);
  }
  if (bad) atomicOr(status, bad);
}

// One thread per (t, m): its whole rows of g_states (cost_bwd_kernel's statements with the factor b_t) and of g_inputs
//   g_inputs[t][j] = a_t (2 (u_t - u*) / l^2 + [t >= 1] 2 (u_t - u_{t-1}) / r^2) - [t + 1 < T] a_{t+1} 2 (u_{t+1} - u_t) / r^2;
// a_{t+1} is recomputed from the particle's rows t + 1 (JOINT mode; ADD: a = G everywhere): no second pass, no atomics.
__global__ void cost_u_bwd_kernel(mcp_cost c, mcp_cost_inputs ci, int T, int M, const double* __restrict__ states,
                                  const double* __restrict__ inputs, const double* __restrict__ g_cost, double gscale,
                                  double* __restrict__ g_states, double* __restrict__ g_inputs) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)T * M) return;
  int t = (int)(i / M);
  const size_t row = (size_t)M * ci.U;  // doubles between a particle's input rows t and t + 1
  const double* x = states + i * c.S;
  const double* u = inputs + i * ci.U;
  const double* up = t > 0 ? u - row : nullptr;
  double* g = g_states + i * c.S;
  const double G = (g_cost ? *g_cost : 1.0) * gscale;
  double e;
  const double a = cost_u_factors(c, ci, x, u, up, t, G, &e);
  for (int s = 0; s < c.S; ++s) g[s] = 0.0;
  if (c.kind == MCP_COST_CARTPOLE) {
    double th = x[c.angle_index];
    double p = (fabs(th) - c.target_angle) / c.ls_angle;
    double b = (x[c.pos_index] - c.target_pos) / c.ls_pos;
    double sg = th > 0.0 ? 1.0 : (th < 0.0 ? -1.0 : 0.0);
    g[c.angle_index] += e * 2.0 * p * sg / c.ls_angle;
    g[c.pos_index] += e * 2.0 * b / c.ls_pos;
  } else if (c.kind == MCP_COST_TRAJ) {
    for (int k = 0; k < c.n_used; ++k) {
      int s = c.used[k];
      double r = (x[s] - c.target_traj[(size_t)t * c.S + s]) / c.lengthscales[k];
      g[s] += e * 2.0 * r / c.lengthscales[k];
    }
  } else {
    for (int k = 0; k < c.n_used; ++k) {
      int s = c.used[k];
      double r = (x[s] - c.target_traj[k]) / c.lengthscales[k];
      g[s] += e * 2.0 * r / c.lengthscales[k];
    }
  }
  if (!g_inputs) return;
  double* gu = g_inputs + i * ci.U;
  for (int j = 0; j < ci.U; ++j) gu[j] = 0.0;
  const bool next = ci.rate_scales && t + 1 < T;
  double an = G;
  if (next && ci.mode != MCP_COST_U_ADD) an = cost_u_factors(c, ci, x + (size_t)M * c.S, u + row, u, t + 1, G, nullptr);
  for (int k = 0; k < ci.n_used; ++k) {
    int j = ci.used[k];
    if (ci.scales) {
      double r = (u[j] - (ci.target ? ci.target[k] : 0.0)) / ci.scales[k];
      gu[j] += a * 2.0 * r / ci.scales[k];
    }
    if (ci.rate_scales && up) {
      double r = (u[j] - up[j]) / ci.rate_scales[k];
      gu[j] += a * 2.0 * r / ci.rate_scales[k];
    }
    if (next) {
      double r = (u[row + j] - u[j]) / ci.rate_scales[k];
      gu[j] -= an * 2.0 * r / ci.rate_scales[k];
    }
  }
}

// ---- time-weighted, risk-sensitive objective (mcp_objective; the project's own extension, include/mcpilco_hip.h) -------------------------
//   J = sum_t w_t (mu_t + kappa sigma_t),  S = sum_t w_t sigma_t,  dJ/dc_tm = w_t [1/n + kappa (c_tm - mu_t) / ((n - 1) sigma_t)]
// over the pooled swarm of n particles.  The per-particle kernels above do not change: the two finalize kernels gain the rows
// (mu_t, sigma_t) and the weights, the two gradient kernels a per-element upstream factor in place of their scalar.

// cost_finalize_kernel, writing rows[t] = (pooled mean, unbiased std) and weighting the two sums: the same Chan pooling and the same
// reduction tree, so that w == NULL, kappa == 0 gives cost_finalize_kernel's bits.
__global__ __launch_bounds__(256) void cost_rows_kernel(int T, int R, const double* __restrict__ moments, RankCounts rc,
                                                        const double* __restrict__ w, double kappa, double* __restrict__ rows,
                                                        double* __restrict__ out) {
  const int64_t* counts = rc.n;
  __shared__ double red[2][4];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  double n_tot = 0.0;
  for (int r = 0; r < R; ++r) n_tot += (double)counts[r];
  double cs = 0.0, ss = 0.0;
  for (int t = tid; t < T; t += 256) {
    double mean = 0.0;
    for (int r = 0; r < R; ++r) mean += (double)counts[r] * moments[((size_t)r * T + t) * 2];
    mean /= n_tot;
    double m2 = 0.0;
    for (int r = 0; r < R; ++r) {
      double d = moments[((size_t)r * T + t) * 2] - mean;
      m2 += moments[((size_t)r * T + t) * 2 + 1] + (double)counts[r] * d * d;
    }
    const double sd = sqrt(m2 / (n_tot - 1.0));
    rows[2 * t] = mean;
    rows[2 * t + 1] = sd;
    double j = mean, s = sd;
    if (kappa != 0.0) j += kappa * sd;
    if (w) {
      j *= w[t];
      s *= w[t];
    }
    cs += j;
    ss += s;
  }
  cs = wave_sum(cs);
  ss = wave_sum(ss);
  if (lane == 0) {
    red[0][wv] = cs;
    red[1][wv] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// cost_finalize_sums_kernel in the same way (the fmax(m2, 0) clamp and mean_out included)
__global__ __launch_bounds__(256) void cost_rows_sums_kernel(int T, double n_tot, const double* __restrict__ sums,
                                                             const double* __restrict__ shift, const double* __restrict__ w, double kappa,
                                                             double* __restrict__ rows, double* __restrict__ out,
                                                             double* __restrict__ mean_out) {
  __shared__ double red[2][4];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  double cs = 0.0, ss = 0.0;
  for (int t = tid; t < T; t += 256) {
    const double a = sums[t], b = sums[T + t];
    const double mean = (shift ? shift[t] : 0.0) + a / n_tot;
    const double m2 = b - a * a / n_tot;
    const double sd = sqrt(fmax(m2, 0.0) / (n_tot - 1.0));
    rows[2 * t] = mean;
    rows[2 * t + 1] = sd;
    double j = mean, s = sd;
    if (kappa != 0.0) j += kappa * sd;
    if (w) {
      j *= w[t];
      s *= w[t];
    }
    cs += j;
    ss += s;
    if (mean_out) mean_out[t] = mean;
  }
  cs = wave_sum(cs);
  ss = wave_sum(ss);
  if (lane == 0) {
    red[0][wv] = cs;
    red[1][wv] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// What a gradient kernel needs of the objective: w and kappa, the forward's costs [T][M], the pooled rows [T][2] and n - 1.
struct ObjectiveArgs {
  const double* w;
  double kappa;
  const double* costs;
  const double* rows;
  double n1;
};

// fac_tm = d J / d c_tm = w_t [1/n + kappa (c_tm - mu_t) / ((n - 1) sigma_t)] for element i = t M + m; gscale = 1/n.  A row of zero spread
// (sigma_t == 0: every particle has the same cost) keeps w_t / n, where autograd through torch.std gives NaN.
__device__ __forceinline__ double objective_factor(const ObjectiveArgs& o, double gscale, size_t i, int t) {
  double fac = gscale;
  if (o.kappa != 0.0) {
    const double sd = o.rows[2 * t + 1];
    if (sd > 0.0) fac += o.kappa * (o.costs[i] - o.rows[2 * t]) / (o.n1 * sd);
  }
  if (o.w) fac *= o.w[t];
  return fac;
}

// the rows of g_states of one (t, m) with the factor e on d d_x / dx: cost_bwd_kernel's statements
__device__ __forceinline__ void state_grad_rows(const mcp_cost& c, const double* x, int t, double e, double* g) {
  for (int s = 0; s < c.S; ++s) g[s] = 0.0;
  if (c.kind == MCP_COST_CARTPOLE) {
    double th = x[c.angle_index];
    double a = (fabs(th) - c.target_angle) / c.ls_angle;
    double b = (x[c.pos_index] - c.target_pos) / c.ls_pos;
    double sg = th > 0.0 ? 1.0 : (th < 0.0 ? -1.0 : 0.0);
    g[c.angle_index] += e * 2.0 * a * sg / c.ls_angle;
    g[c.pos_index] += e * 2.0 * b / c.ls_pos;
  } else if (c.kind == MCP_COST_TRAJ) {
    for (int k = 0; k < c.n_used; ++k) {
      int s = c.used[k];
      double r = (x[s] - c.target_traj[(size_t)t * c.S + s]) / c.lengthscales[k];
      g[s] += e * 2.0 * r / c.lengthscales[k];
    }
  } else {
    for (int k = 0; k < c.n_used; ++k) {
      int s = c.used[k];
      double r = (x[s] - c.target_traj[k]) / c.lengthscales[k];
      g[s] += e * 2.0 * r / c.lengthscales[k];
    }
  }
}

// cost_bwd_kernel with the per-element factor: one thread per (t, m), its whole row
__global__ void cost_bwd_shaped_kernel(mcp_cost c, ObjectiveArgs o, int T, int M, const double* __restrict__ states,
                                       const double* __restrict__ g_cost, double gscale, double* __restrict__ g_states) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)T * M) return;
  int t = (int)(i / M);
  const double* x = states + i * c.S;
  double dist;
  cost_point(c, x, t, &dist);
  double e = (g_cost ? *g_cost : 1.0) * objective_factor(o, gscale, i, t);
  if (c.kind != MCP_COST_TARGET_QUAD) e *= exp(-dist);
  state_grad_rows(c, x, t, e, g_states + i * c.S);
}

// cost_u_bwd_kernel with the per-element factor.  The rate term couples rows t and t + 1 of a particle, and the factor now differs between
// them: a_{t+1} is built from G_{t+1,m} -- row t + 1 of costs, rows and w --, not from this element's G.
__global__ void cost_u_bwd_shaped_kernel(mcp_cost c, mcp_cost_inputs ci, ObjectiveArgs o, int T, int M, const double* __restrict__ states,
                                         const double* __restrict__ inputs, const double* __restrict__ g_cost, double gscale,
                                         double* __restrict__ g_states, double* __restrict__ g_inputs) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)T * M) return;
  int t = (int)(i / M);
  const size_t row = (size_t)M * ci.U;
  const double* x = states + i * c.S;
  const double* u = inputs + i * ci.U;
  const double* up = t > 0 ? u - row : nullptr;
  const double g0 = g_cost ? *g_cost : 1.0;
  const double G = g0 * objective_factor(o, gscale, i, t);
  double e;
  const double a = cost_u_factors(c, ci, x, u, up, t, G, &e);
  state_grad_rows(c, x, t, e, g_states + i * c.S);
  if (!g_inputs) return;
  double* gu = g_inputs + i * ci.U;
  for (int j = 0; j < ci.U; ++j) gu[j] = 0.0;
  const bool next = ci.rate_scales && t + 1 < T;
  double an = G;
  if (next) {
    an = g0 * objective_factor(o, gscale, i + M, t + 1);
    if (ci.mode != MCP_COST_U_ADD) an = cost_u_factors(c, ci, x + (size_t)M * c.S, u + row, u, t + 1, an, nullptr);
  }
  for (int k = 0; k < ci.n_used; ++k) {
    int j = ci.used[k];
    if (ci.scales) {
      double r = (u[j] - (ci.target ? ci.target[k] : 0.0)) / ci.scales[k];
      gu[j] += a * 2.0 * r / ci.scales[k];
    }
    if (ci.rate_scales && up) {
      double r = (u[j] - up[j]) / ci.rate_scales[k];
      gu[j] += a * 2.0 * r / ci.rate_scales[k];
    }
    if (next) {
      double r = (u[row + j] - u[j]) / ci.rate_scales[k];
      gu[j] -= an * 2.0 * r / ci.rate_scales[k];
    }
  }
}

extern "C" int mcp_cost_fwd(const mcp_cost* cost, int T, int M, const double* states, double* costs, double* moments, uint32_t* status,
                            void* stream) {
  if (!cost_ok(cost) || !states || !costs || !moments || !status || T <= 0 || M <= 0) return MCP_ERR_ARG;
  hipLaunchKernelGGL(cost_fwd_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, *cost, T, M, states, costs, moments, status);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cost_finalize(int T, int R, const double* moments, const int64_t* counts, double* out, void* stream) {
  if (!moments || !counts || !out || T <= 0 || R <= 0) return MCP_ERR_ARG;
  if (R > 64) return MCP_ERR_LIMIT;
  RankCounts rc;
  for (int r = 0; r < 64; ++r) rc.n[r] = r < R ? counts[r] : 0;
  hipLaunchKernelGGL(cost_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, T, R, moments, rc, out);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cost_sums(int T, int M, const double* moments, const double* shift, double* sums, void* stream) {
  if (!moments || !sums || T <= 0 || M <= 0) return MCP_ERR_ARG;
  hipLaunchKernelGGL(cost_sums_kernel, dim3((T + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, (double)M, moments, shift, sums);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cost_finalize_sums(int T, int64_t n_total, const double* sums, const double* shift, double* out, double* mean_out,
                                      void* stream) {
  if (!sums || !out || T <= 0 || n_total <= 0) return MCP_ERR_ARG;
  hipLaunchKernelGGL(cost_finalize_sums_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, T, (double)n_total, sums, shift, out, mean_out);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cost_bwd(const mcp_cost* cost, int T, int M, const double* states, const double* g_cost, double gscale,
                            double* g_states, void* stream) {
  if (!cost_ok(cost) || !states || !g_states || T <= 0 || M <= 0) return MCP_ERR_ARG;
  size_t n = (size_t)T * M;
  hipLaunchKernelGGL(cost_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *cost, T, M, states, g_cost,
                     gscale, g_states);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cost_u_fwd(const mcp_cost* cost, const mcp_cost_inputs* cin, int T, int M, const double* states, const double* inputs,
                              double* costs, double* moments, uint32_t* status, void* stream) {
  if (!cost_ok(cost) || !cost_inputs_ok(cin)) return MCP_ERR_ARG;
  if (cost_inputs_none(cin)) return mcp_cost_fwd(cost, T, M, states, costs, moments, status, stream);
  if (!states || !inputs || !costs || !moments || !status || T <= 0 || M <= 0) return MCP_ERR_ARG;
  hipLaunchKernelGGL(cost_u_fwd_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, *cost, *cin, T, M, states, inputs, costs, moments,
                     status);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cost_u_bwd(const mcp_cost* cost, const mcp_cost_inputs* cin, int T, int M, const double* states, const double* inputs,
                              const double* g_cost, double gscale, double* g_states, double* g_inputs, void* stream) {
  if (!cost_ok(cost) || !cost_inputs_ok(cin)) return MCP_ERR_ARG;
  if (cost_inputs_none(cin)) {
    // (no descriptor, no U: the width of g_inputs is then unknown, so it cannot be given)
    if ((g_inputs && !cin) || !states || !g_states || T <= 0 || M <= 0) return MCP_ERR_ARG;
    if (g_inputs && hipMemsetAsync(g_inputs, 0, (size_t)T * M * cin->U * sizeof(double), (hipStream_t)stream) != hipSuccess)
      return MCP_ERR_LAUNCH;
    return mcp_cost_bwd(cost, T, M, states, g_cost, gscale, g_states, stream);
  }
  if (!states || !inputs || !g_states || T <= 0 || M <= 0) return MCP_ERR_ARG;
  size_t n = (size_t)T * M;
  hipLaunchKernelGGL(cost_u_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *cost, *cin, T, M, states,
                     inputs, g_cost, gscale, g_states, g_inputs);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

// the objective, when there is one: a finite kappa, and two particles or more where the std term is on
static bool objective_ok(const mcp_objective* obj, int64_t n_total) {
  if (!obj) return true;
  if (!std::isfinite(obj->kappa)) return false;
  return obj->kappa == 0.0 || n_total >= 2;
}

extern "C" int mcp_cost_rows(int T, int R, const double* moments, const int64_t* counts, const mcp_objective* obj, double* rows,
                             double* out, void* stream) {
  if (!moments || !counts || !rows || !out || T <= 0 || R <= 0) return MCP_ERR_ARG;
  if (R > 64) return MCP_ERR_LIMIT;
  RankCounts rc;
  int64_t n_total = 0;
  for (int r = 0; r < 64; ++r) {
    rc.n[r] = r < R ? counts[r] : 0;
    n_total += rc.n[r];
  }
  if (!objective_ok(obj, n_total)) return MCP_ERR_ARG;
  hipLaunchKernelGGL(cost_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, T, R, moments, rc, obj ? obj->w : nullptr,
                     obj ? obj->kappa : 0.0, rows, out);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cost_rows_sums(int T, int64_t n_total, const double* sums, const double* shift, const mcp_objective* obj, double* rows,
                                  double* out, double* mean_out, void* stream) {
  if (!sums || !rows || !out || T <= 0 || n_total <= 0 || !objective_ok(obj, n_total)) return MCP_ERR_ARG;
  hipLaunchKernelGGL(cost_rows_sums_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, T, (double)n_total, sums, shift,
                     obj ? obj->w : nullptr, obj ? obj->kappa : 0.0, rows, out, mean_out);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_cost_bwd_shaped(const mcp_cost* cost, const mcp_cost_inputs* cin, const mcp_objective* obj, int T, int M,
                                   int64_t n_total, const double* states, const double* inputs, const double* costs, const double* rows,
                                   const double* g_cost, double* g_states, double* g_inputs, void* stream) {
  if (cin && cin->U > MCP_MAX_INPUT) return MCP_ERR_LIMIT;
  if (!cost_ok(cost) || !cost_inputs_ok(cin)) return MCP_ERR_ARG;
  if (!states || !costs || !rows || !g_states || T <= 0 || M <= 0 || n_total < M || !objective_ok(obj, n_total)) return MCP_ERR_ARG;
  const ObjectiveArgs o = {obj ? obj->w : nullptr, obj ? obj->kappa : 0.0, costs, rows, (double)(n_total - 1)};
  const double gscale = 1.0 / (double)n_total;
  const size_t n = (size_t)T * M;
  if (cost_inputs_none(cin)) {
    if (g_inputs && !cin) return MCP_ERR_ARG;  // (no descriptor, no U: as mcp_cost_u_bwd)
    if (g_inputs && hipMemsetAsync(g_inputs, 0, n * cin->U * sizeof(double), (hipStream_t)stream) != hipSuccess) return MCP_ERR_LAUNCH;
    hipLaunchKernelGGL(cost_bwd_shaped_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *cost, o, T, M, states,
                       g_cost, gscale, g_states);
    MCP_LAUNCH_CHECK();
    return MCP_OK;
  }
  if (!inputs) return MCP_ERR_ARG;
  hipLaunchKernelGGL(cost_u_bwd_shaped_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *cost, *cin, o, T, M,
                     states, inputs, g_cost, gscale, g_states, g_inputs);
  MCP_LAUNCH_CHECK();
  return MCP_OK;
}

extern "C" int mcp_abi_version(void) { return MCP_ABI_VERSION; }
extern "C" const char* mcp_build_info(void) { return "libmcpilco_hip gfx950 fp64 (" __DATE__ " " __TIME__ ")"; }
