/*
 * md_expert_sense.h -- the PPO expert observing through its OWN sensors (numpy_expert.py:39-62: expert(vehicle) builds a
 * LidarStateObservation of its own -- 240 lasers at 50 m, num_others = 4, no noise, no detectors, random_agent_model off --
 * and observes the vehicle through it on every call), so that the expert drives envs of any vehicle config and the
 * multi-agent envs.  md_expert (include/md_expert.h) assembles the expert's vector from the env's obs row and is limited to
 * the configs where that row already is the expert's; md_expert_sense reads nothing but the live state.
 *
 * One launch; one 4-wave workgroup per tile of 16 ROWS, row i = agent i % agents_per_env of env i / agents_per_env (a tile
 * may straddle envs).  For every row of an env with need_reset == 0 the kernel builds the expert's 275-vector in LDS:
 *   state  [0, 19)    md_observe_ctx + tasks 0, 1, 2, 3, 4, 8 of md_observe_task on lanes of a wave, assembled by
 *                     md_observe_state_dims under the expert's layout config
 *   others [19, 35)   md_others_block (num_others = 4) on the row's own detected sets
 *   cloud  [35, 275)  the step kernels' lidar cast (one wave per row and 64-beam sector, items taken by LDS ticket) against
 *                     the env's shape table, read through L2; the detected sets are two 64-bit words per row in LDS
 * then md_expert_correct, the MLP of md_expert (the same tile code, the same chains) and the action.
 * The expert's layout config is the caller's MdConfig with n_beams = 240, lidar_range = 50, n_side = n_lane_line = 0,
 * random_agent_model = 0, num_others = 4, add_others_navi = 0, obs_dim = 275.
 *
 * The uncorrected row is, bit for bit, the obs row md_step would have left for that agent had the batch been configured
 * with the expert's sensor config (slots that hold no driving agent included).  The env's own lidar noise / dropout never
 * touch it.  Nothing of MdState is written; MdState.obs and MdState.detected are not read.
 *
 * Rows of an env with need_reset != 0 are not sensed (the next md_step restores that env and ignores the action; after
 * md_swap_draw its nav indices no longer belong to the map env_map names): action, mlp and obs rows are zeros.
 *
 * Refused: traffic_mode 4 (scenario mode) and ma_kind = MD_MA_TOLLGATE (its observation has no navigation dims).
 */
#ifndef MD_EXPERT_SENSE_H
#define MD_EXPERT_SENSE_H

#include "md_expert.h"

#define MD_EXPERT_BEAMS 240       /* the expert's lidar */
#define MD_EXPERT_RANGE 50.0f

#ifdef __cplusplus
extern "C" {
#endif
/* rows = n_envs * agents_per_env.
 *   weights      MD_EXPERT_NW packed floats, 16-byte aligned
 *   beam_cs240   240 x (cos, sin): the expert's beam table (what MdWorld.beam_cs is for a 240-beam lidar), 16-byte aligned
 *   noise        [rows][2] N(0, 1) draws, or NULL = the mean (deterministic)
 *   action_out   [rows][2]
 *   mlp_out      [rows][4] mean | log_std, or NULL
 *   obs_out      [rows][275] the corrected vector, or NULL
 * Returns MD_OK or an error (md_last_error). */
int md_expert_sense(const MdWorld* w, const MdState* s, const MdConfig* c, const float* weights, const float* beam_cs240,
                    const float* noise, float* action_out, float* mlp_out, float* obs_out, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* MD_EXPERT_SENSE_H */
