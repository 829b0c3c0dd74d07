/*
 * mcpilco_hip_debug.h -- test and diagnostic entry points of libmcpilco_hip.so.  NOT part of the drop-in boundary
 * (include/mcpilco_hip.h): the product path never needs them.  They exist so that the parity tests can force every kernel variant the
 * automatic dispatch of mcp_rollout_fwd / mcp_rollout_bwd / mcp_posterior_fwd may choose, so that bench.py / tools can report which
 * variant ran, and so that tools/phase_stamps.py can read per-phase cycle counters.  (mcp_chol_factor / mcp_chol_inverse have one path
 * per size and no `_ex` form.)
 *
 * Round 5: the request travels WITH THE CALL.  Every `_ex` entry point is its plain namesake plus a `mcp_dispatch*` (NULL or all zero =
 * automatic: the plain entry points pass NULL); the library keeps no dispatch state of its own -- no setters, nothing process-wide.
 */
#ifndef MCPILCO_HIP_DEBUG_H
#define MCPILCO_HIP_DEBUG_H

#include "mcpilco_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcp_dispatch {
  /* ---- requests (0 = automatic) ---- */
  int32_t fwd_particles; /* forward: particles per workgroup 1 / 2 / 4 (small-tile kernels) or 16 (matrix-core tile kernel)                 */
  int32_t gp_sharding;   /* GP-sharded launch forms: 1 never, 2 whenever the grid fits the device                                        */
  int32_t fwd_lean;      /* the latency-lean GP-sharded kernel (rollout_fwd_lat_kernel): 1 never                                        */
  int32_t policy_split;  /* GP-sharded 16-particle kernel: 1 every member evaluates the whole policy, 2 split whenever the shape allows */
  int32_t row_split;     /* GP-sharded 16-particle kernel: 1 one workgroup per (tile, GP range), 2 / 3 that many (row parts of Kinv) whenever allowed */
  int32_t cluster_map;   /* ... its row-split form: 1 the workgroups of a tile on one XCD, 2 dealt row part major                        */
  int32_t fwd_no_xlds;   /* small-tile kernel: 1 never stage the small operands in LDS                                                  */
  int32_t fwd_gb;        /* small-tile kernel: GPs per pass (0 = as many as fit)                                                        */
  int32_t bwd_particles; /* backward sweep: particles per workgroup 1 / 2 / 4 / 8 (forces the general sweep)                            */
  int32_t bwd_lean;      /* the latency-lean sweep (rollout_bwd_lat_kernel): 1 never                                                    */
  int32_t bwd_pipe;      /* general sweep, one particle per workgroup on the wide classes: 1 never the pipelined form (chain beside the RBF stage) */
  uint32_t stamp_block;  /* which workgroup of the forward launch writes its stamps                                                     */
  void* fwd_stamps;      /* device buffer of 64 uint64 per-phase cycle totals of that workgroup (NULL = off)                            */
  void* bwd_stamps;      /* device buffer of 16 uint64 (backward sweep)                                                                 */
  /* ---- report (written by the call) ---- */
  int32_t ran_particles;  /* forward / posterior: particles per workgroup launched (16 = tile kernel) */
  int32_t ran_gp_sharded; /* number of GP-sharded launches the forward call made (0 = unsharded)      */
  int32_t ran_fwd_lean;   /* 1: the lean forward kernel ran                                           */
  int32_t ran_bwd_lean;   /* 1: the lean backward sweep ran                                           */
  int32_t ran_row_split;  /* 2 / 3: the forward launch put that many workgroups on every (tile, GP range) */
  int32_t ran_bwd_pipe;   /* 1: the general sweep ran in its pipelined form                              */
} mcp_dispatch;

int mcp_rollout_fwd_ex(const mcp_model* model, const mcp_policy* policy, const mcp_noise* noise, int M, int T, int particle_pred,
                       const double* x0, double* states, double* inputs, double* jac, uint32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream, mcp_dispatch* d);
int mcp_rollout_bwd_ex(const mcp_model* model, const mcp_policy* policy, const mcp_noise* noise, int M, int T, const double* states,
                       const double* inputs, const double* jac, const double* g_states, const double* g_inputs, double* g_log_ls,
                       double* g_centers, double* g_weight, double* g_x0, void* workspace, size_t workspace_bytes, void* stream,
                       mcp_dispatch* d);
int mcp_posterior_fwd_ex(const mcp_gp* gp, int M, const double* Z, double* mu, double* var, double* Jmu, double* Jvar, uint32_t* status,
                         void* stream, mcp_dispatch* d);

/*
 * Plan queries: what mcp_rollout_fwd_ex / mcp_rollout_bwd_ex would decide for a call, without making it.  Same descriptors, M, T, flags
 * (the particle_pred argument) and workspace size (0 = no workspace), the device's compute-unit count given explicitly, and a request
 * (NULL = automatic).  They return what the real call returns from validating its descriptors and planning, read only the scalars of the
 * descriptors (pointers are tested for NULL, never followed) and make no HIP call: they run on a machine without a GPU.  All fields int32.
 */
enum { MCP_FWD_SMALL_SHARDED = 1, MCP_FWD_LEAN = 2, MCP_FWD_TILE_SHARDED = 3, MCP_FWD_TILE = 4, MCP_FWD_SMALL = 5 };
typedef struct mcp_fwd_plan {
  int32_t family;               /* MCP_FWD_*: small-tile kernel GP-sharded, lean kernel, 16-particle kernel GP-sharded, 16-particle, small-tile */
  int32_t particles;            /* particles per workgroup */
  int32_t xlds, gb, ncmax;      /* small-tile kernels: operands staged in LDS, GPs per pass, column chunks per pass */
  int32_t lds_bytes;            /* dynamic LDS of the small-tile and lean kernels (the 16-particle kernel sizes its own) */
  int32_t npad_max, maxdeg;     /* of the model: largest padded training set, highest polynomial degree */
  int32_t launches;             /* kernel launches of the rollout proper */
  int32_t particles_per_launch;
  int32_t gsh_cs, gsh_rs, gsh_map, policy_split; /* GP-sharded 16-particle launch: workgroups per tile, row parts, deal, policy split */
  int32_t ws_xch, ws_xj, ws_kt, ws_uxch, ws_rxch, ws_total; /* the forward workspace map: byte offsets of its regions and their end (capped at INT32_MAX) */
  int32_t use_xj, use_kt;       /* the caller's workspace reaches the packed phase-J operands / the lean kernel's Kinv tiles */
  int32_t zero_xch, zero_uxch, zero_rxch;        /* granule regions zeroed on the stream before the launch */
  int32_t pack_kt, pack_xj;     /* operand packs built on the stream before the launch */
  int32_t ran_particles, ran_gp_sharded, ran_fwd_lean, ran_row_split; /* the report words the call writes */
} mcp_fwd_plan;
typedef struct mcp_bwd_plan {
  int32_t lean;                 /* 1: the latency-lean sweep */
  int32_t pfm, um;              /* sweep class <PFM, UM> */
  int32_t maxnt;                /* thread class of the general sweep: 256 / 512 / 1024 (0: lean) */
  int32_t particles;            /* particles per workgroup (lean: its two slots) */
  int32_t threads;              /* threads per workgroup */
  int32_t pipe;                 /* general sweep: the pipelined form */
  int32_t launches;
  int32_t slabs;                /* per-workgroup gradient slabs the reduction sums */
  int32_t ran_bwd_lean, ran_bwd_pipe; /* the report words the call writes */
} mcp_bwd_plan;
int mcp_rollout_fwd_plan(const mcp_model* model, const mcp_policy* policy, int M, int T, int particle_pred, size_t workspace_bytes, int cus,
                         const mcp_dispatch* request, mcp_fwd_plan* plan);
int mcp_rollout_bwd_plan(const mcp_model* model, const mcp_policy* policy, int M, int T, int particle_pred, size_t workspace_bytes, int cus,
                         const mcp_dispatch* request, mcp_bwd_plan* plan);

/*
 * The training epoch's plan: where mcp_nll_epoch keeps what it makes inside its workspace and which gradient form it launches for
 * (G, N, D).  Returns what mcp_nll_epoch returns from validating the three sizes; no HIP call.  All fields int64.  Offsets in doubles:
 * `first_gp` from the start of the workspace (the G mcp_kernel descriptors come first), GP g's block at first_gp + g per_gp, the others
 * inside a GP's block, in the order K -> U | Uinv | Kinv | alpha | r | slab | grad | inv_ls | w1 | w20 | w21 | scal | logdet.
 */
enum { MCP_NLL_GRAD_ROWS = 1, MCP_NLL_GRAD_ROW_PER_WG = 2 };
typedef struct mcp_nll_plan {
  int64_t first_gp, per_gp, total; /* total: the whole workspace = mcp_nll_epoch_workspace_bytes / 8 */
  int64_t K, Uinv, Kinv, alpha, r, slab, grad, inv_ls, w1, w20, w21, scal, logdet;
  int64_t grad_form;   /* MCP_NLL_GRAD_ROWS: inputs in LDS, rows_per_wg rows per workgroup; MCP_NLL_GRAD_ROW_PER_WG: one workgroup per row of K */
  int64_t rows_per_wg; /* rows of K per workgroup of the gradient launch */
  int64_t slab_rows;   /* rows of the slab the finish kernel adds: workgroups of the gradient launch per GP */
  int64_t lds_bytes;   /* dynamic LDS of the gradient launch */
} mcp_nll_plan;
int mcp_nll_epoch_plan(int G, int N, int D, mcp_nll_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* MCPILCO_HIP_DEBUG_H */
