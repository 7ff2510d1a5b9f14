// parts/others.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: others_kernel, which md_step launches after its step kernel when num_others > 0.
// Relies on: the headers only (md_others_block).

namespace {

// "Others" block of the observation (Lidar.get_surrounding_vehicles_info): one thread per agent, after the
// step kernel has written the detected sets and the new state back.  Off in the headline configs.
__global__ __launch_bounds__(64) void others_kernel(MdWorld w, MdState g, MdConfig c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_envs * c.agents_per_env) return;
    const int e = i / c.agents_per_env, a = i - e * c.agents_per_env;
    const MdState s = md_env_view(&g, &c, e);
    const int m = w.env_map[e];
    md_others_block(w.lanes + w.lane_off[m], w.roads + w.road_off[m], &s, &c, a, s.detected[2 * a], s.detected[2 * a + 1],
                    s.obs + (size_t)a * c.obs_dim + md_obs_others(&c));
}

}  // namespace
