// The HISTORY forms of the fused closed loop under the tanh MLP (mcp_rollout_mlp_hist, mcp_rollout_mlp_hist_bwd): the network reads a window of
// the last h rows.  The kernel templates are rollout_mlp_kernels.h's (template HIST: the account of the forward form and of the sweep is
// there); this translation unit instantiates them -- the forward ladder and the sweep with and without the weights' LDS copy -- so that
// they compile beside the family's other forms and not behind them.  On the true state only: a measured form ran into a GPU fault whose
// cause was not found and is not built (the entries refuse hist with a measurement model).  rollout_mlp.hip's dispatchers make the checks
// and fill the arguments, then call the two functions below.
#include "rollout_mlp_kernels.h"

namespace mcp {

int launch_mlp_hist(const OpenArgsMlpMeas& a, double p_drop, const mcp_mlp_track* trk, const mcp_mlp_pd* res, const mcp_mlp_hist* hist, int maxdeg,
                    bool wantvar, hipStream_t st) {
  return launch_mlp_tiles<false, true, true, true, true>(mlp_with_hist<OpenArgsMlpHist<false>, OpenArgsMlp>(a, p_drop, trk, res, hist), maxdeg, wantvar, st);
}

int launch_mlp_hist_bwd(const MlpBwdArgsMeas& a, const mcp_noise* noise, double p_drop, const mcp_mlp_track* trk, const mcp_mlp_pd* res,
                        const mcp_mlp_hist* hist, size_t lds, hipStream_t st) {
  return launch_mlp_bwd_hist(a, noise, p_drop, trk, res, hist, lds, st);
}

}  // namespace mcp
