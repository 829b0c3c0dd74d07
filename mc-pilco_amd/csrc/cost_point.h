// The point costs of the cost kernels (cost.hip) and of the planner's rollout (mppi.hip), and the descriptor checks of their entries: one text,
// instantiated by both sources -- the library is built without floating-point contraction, so a (state, input) row costs the same bits in either.
#pragma once
#include "mcp_device.h"

#include <cmath>

using namespace mcp;

__device__ __forceinline__ double cost_point(const mcp_cost& c, const double* x, int t, double* dist_out) {
  double dist = 0.0;
  if (c.kind == MCP_COST_CARTPOLE) {
    double a = (fabs(x[c.angle_index]) - c.target_angle) / c.ls_angle;
    double b = (x[c.pos_index] - c.target_pos) / c.ls_pos;
    dist = a * a + b * b;
  } else if (c.kind == MCP_COST_TRAJ) {
    for (int i = 0; i < c.n_used; ++i) {
      int s = c.used[i];
      double r = (x[s] - c.target_traj[(size_t)t * c.S + s]) / c.lengthscales[i];
      dist = fma(r, r, dist);
    }
  } else {  // MCP_COST_TARGET / _QUAD: ONE target row [n_used], the same at every t
    for (int i = 0; i < c.n_used; ++i) {
      double r = (x[c.used[i]] - c.target_traj[i]) / c.lengthscales[i];
      dist = fma(r, r, dist);
    }
  }
  if (dist_out) *dist_out = dist;
  if (c.kind == MCP_COST_TARGET_QUAD) return dist;
  return 1.0 - exp(-dist);
}

// ---- control-effort and input-rate terms (mcp_cost_inputs; the project's own extension, include/mcpilco_hip.h) ------------------------
// d_u = sum_i ((u[idx_i] - u*_i) / l_i)^2 and d_r = sum_i ((u[idx_i] - up[idx_i]) / r_i)^2 (up: the particle's row t - 1, NULL at t = 0),
// each absent (0) without its scales; summed in index order like cost_point's distance.
__device__ __forceinline__ void input_dist(const mcp_cost_inputs& ci, const double* u, const double* up, double* du_out, double* dr_out) {
  double du = 0.0, dr = 0.0;
  if (ci.scales)
    for (int i = 0; i < ci.n_used; ++i) {
      double r = (u[ci.used[i]] - (ci.target ? ci.target[i] : 0.0)) / ci.scales[i];
      du = fma(r, r, du);
    }
  if (ci.rate_scales && up)
    for (int i = 0; i < ci.n_used; ++i) {
      double r = (u[ci.used[i]] - up[ci.used[i]]) / ci.rate_scales[i];
      dr = fma(r, r, dr);
    }
  *du_out = du;
  *dr_out = dr;
}

// MCP_COST_U_ADD: f(d_x) + d_u + d_r;  MCP_COST_U_JOINT: f(d_x + d_u + d_r)
__device__ __forceinline__ double cost_u_point(const mcp_cost& c, const mcp_cost_inputs& ci, const double* x, const double* u, const double* up,
                                               int t) {
  double dx, du, dr;
  const double fx = cost_point(c, x, t, &dx);
  input_dist(ci, u, up, &du, &dr);
  if (ci.mode == MCP_COST_U_ADD) return (fx + du) + dr;
  const double d = (dx + du) + dr;
  if (c.kind == MCP_COST_TARGET_QUAD) return d;
  return 1.0 - exp(-d);
}

static bool cost_ok(const mcp_cost* c) {
  if (!c || c->S <= 0 || c->S > MCP_MAX_STATE) return false;
  if (c->kind == MCP_COST_CARTPOLE)
    return c->angle_index >= 0 && c->angle_index < c->S && c->pos_index >= 0 && c->pos_index < c->S && c->ls_angle != 0.0 &&
           c->ls_pos != 0.0;
  if (c->kind == MCP_COST_TRAJ || c->kind == MCP_COST_TARGET || c->kind == MCP_COST_TARGET_QUAD) {
    if (c->n_used <= 0 || c->n_used > MCP_MAX_STATE || !c->target_traj || !c->lengthscales) return false;
    for (int i = 0; i < c->n_used; ++i)
      if (c->used[i] < 0 || c->used[i] >= c->S) return false;
    return true;
  }
  return false;
}

// the inputs descriptor, when there is one: sizes, mode, distinct indices inside [0, U)
static bool cost_inputs_ok(const mcp_cost_inputs* ci) {
  if (!ci) return true;
  if (ci->U < 1 || ci->U > MCP_MAX_INPUT || ci->n_used < 0 || ci->n_used > MCP_MAX_INPUT) return false;
  if (ci->mode != MCP_COST_U_ADD && ci->mode != MCP_COST_U_JOINT) return false;
  for (int i = 0; i < ci->n_used; ++i) {
    if (ci->used[i] < 0 || ci->used[i] >= ci->U) return false;
    for (int k = 0; k < i; ++k)
      if (ci->used[k] == ci->used[i]) return false;
  }
  return true;
}
static bool cost_inputs_none(const mcp_cost_inputs* ci) { return !ci || ci->n_used == 0 || (!ci->scales && !ci->rate_scales); }
