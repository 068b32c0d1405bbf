"""ctypes binding of libgmpe.so (include/gmpe.h). No CPU fallback: a missing library raises."""
import ctypes as C
import os

from .config import GmpeConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
# GMPE_LIB: diagnostic override to A/B another build of the SAME library (tools/*.py); never a fallback. bench.py refuses to report
# a number with it set (unless --diag, which records it in the JSON line).
LIB_PATH = os.environ.get("GMPE_LIB") or os.path.join(_HERE, "libgmpe.so")
_lib = None

SYMBOLS = ["gmpe_abi_version", "gmpe_last_error", "gmpe_obs_dim", "gmpe_node_feats", "gmpe_num_entities", "gmpe_create",
           "gmpe_destroy", "gmpe_set_rng_tape", "gmpe_reset", "gmpe_step", "gmpe_step_many", "gmpe_step_many_prepare", "gmpe_step_onehot",
           "gmpe_field_bytes", "gmpe_get_field", "gmpe_set_field", "gmpe_edges_from_adj", "gmpe_masks_from_dones",
           "gmpe_timing_enable", "gmpe_timing_read", "gmpe_timing_mark", "gmpe_timing_region_ms",
           "gmpe_rollout_steps", "gmpe_get_tuning", "gmpe_step_many_launches", "gmpe_edges_from_adj_compact",
           "gmpe_set_control_override", "gmpe_field_device_ptr", "gmpe_step_envs", "gmpe_step_many_envs",
           "gmpe_entity_table_width", "gmpe_expand_node_obs", "gmpe_expand_adj",
           "gmpe_returns_workspace_bytes", "gmpe_compute_returns", "gmpe_available_actions_from_dones", "gmpe_minibatch_gather",
           "gmpe_insert_learner", "gmpe_episode_record", "gmpe_episode_metrics", "gmpe_episode_summary",
           "gmpe_minibatch_edges", "gmpe_minibatch_edges_workspace_bytes", "gmpe_episode_record_series",
           "gmpe_ppo_loss", "gmpe_ppo_loss_workspace_bytes", "gmpe_ppo_loss_popart", "gmpe_ppo_loss_popart_workspace_bytes",
           "gmpe_act_sample", "gmpe_compute_returns_shard", "gmpe_ppo_loss_shard",
           "gmpe_gru_workspace_bytes", "gmpe_gru_forward", "gmpe_gru_backward",
           "gmpe_mlp_workspace_bytes", "gmpe_mlp_forward", "gmpe_mlp_backward",
           "gmpe_gnn_workspace_bytes", "gmpe_gnn_forward", "gmpe_gnn_backward", "gmpe_gnn_forward_table", "gmpe_gnn_backward_table",
           "gmpe_gnn_forward_wide", "gmpe_gnn_forward_wide_table", "gmpe_gnn_wide_geometry",
           "gmpe_head_workspace_bytes", "gmpe_head_forward", "gmpe_head_backward", "gmpe_act_head",
           "gmpe_value_workspace_bytes", "gmpe_value_forward", "gmpe_value_backward",
           "gmpe_optim_workspace_bytes", "gmpe_optim_step", "gmpe_optim_shard_elems", "gmpe_optim_step_shard",
           "gmpe_optim_schedule_bytes", "gmpe_optim_schedule_fill", "gmpe_optim_step_scheduled",
           "gmpe_env_infos", "gmpe_eval_step", "gmpe_eval_mean", "gmpe_step_tail"]


class GmpeOutputs(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("agent_id", C.c_void_p), ("node_obs", C.c_void_p),
                ("adj", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("info", C.c_void_p), ("adj_compact", C.c_int32), ("reserved", C.c_int32), ("entity_table", C.c_void_p)]


class GmpeRollout(C.Structure):
    """gmpe_rollout (include/gmpe.h): K steps in one launch, step k -> output slot (first_slot + k) % num_slots."""
    _fields_ = [("num_steps", C.c_int32), ("num_action_sets", C.c_int32), ("num_slots", C.c_int32), ("first_slot", C.c_int32),
                ("stride_obs", C.c_int64), ("stride_agent_id", C.c_int64), ("stride_node_obs", C.c_int64), ("stride_adj", C.c_int64),
                ("stride_reward", C.c_int64), ("stride_done", C.c_int64), ("stride_info", C.c_int64), ("stride_masks", C.c_int64),
                ("masks", C.c_void_p), ("active_masks", C.c_void_p), ("stride_entity_table", C.c_int64)]


class GmpeTuning(C.Structure):
    _fields_ = [("G", C.c_int32), ("block", C.c_int32), ("nt", C.c_int32), ("spec", C.c_int32), ("split", C.c_int32),
                ("roll", C.c_int32), ("ap", C.c_int32), ("lds_bytes", C.c_int32), ("diag_build", C.c_int32),
                ("G_roll", C.c_int32), ("block_roll", C.c_int32), ("chunks", C.c_int32), ("ahead", C.c_int32), ("xstep", C.c_int32), ("chunks_x", C.c_int32), ("ahead_x", C.c_int32),
                ("lds_bytes_roll", C.c_int32)]


class GmpeReturnsPlan(C.Structure):
    """gmpe_returns_plan (include/gmpe.h): GraphReplayBuffer.compute_returns + GR_MAPPO.train's advantages, handle-less."""
    _fields_ = [("num_steps", C.c_int32), ("flags", C.c_int32), ("lanes", C.c_int64), ("stride", C.c_int64),
                ("gamma", C.c_double), ("gae_lambda", C.c_double),
                ("rewards", C.c_void_p), ("masks", C.c_void_p), ("bad_masks", C.c_void_p), ("value_preds", C.c_void_p), ("returns", C.c_void_p),
                ("next_value", C.c_void_p), ("denorm_mean", C.c_void_p), ("denorm_std", C.c_void_p), ("advantages", C.c_void_p),
                ("active_masks", C.c_void_p), ("normalized", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


RETURNS_GAE, RETURNS_PROPER_TIME_LIMITS, RETURNS_ADVANTAGES_ONLY = 1, 2, 4
SHARD_LOCAL, SHARD_APPLY, SHARD_MAX_WORLD = 0, 1, 4096
RETURNS_SHARD_STATS, PPO_SHARD_STATS = 3, 4


class GmpeReturnsShardPlan(C.Structure):
    """gmpe_returns_shard_plan (include/gmpe.h): gmpe_returns_plan in two phases around an exchange of the shards' (n, mean, M2)."""
    _fields_ = [("base", GmpeReturnsPlan), ("phase", C.c_int32), ("world", C.c_int32), ("local", C.c_void_p), ("all", C.c_void_p)]


class GmpeAvailPlan(C.Structure):
    """gmpe_avail_plan (include/gmpe.h): the stop-action rows of available_actions from the previous step's dones."""
    _fields_ = [("dones", C.c_void_p), ("available_actions", C.c_void_p), ("lanes", C.c_int64), ("n_actions", C.c_int32),
                ("num_positions", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("stride_dones", C.c_int64), ("stride_out", C.c_int64)]


class GmpeLearnerPlan(C.Structure):
    """gmpe_learner_plan (include/gmpe.h): the policy's outputs of one step into the rollout buffer's slots, done rows of the RNN states zeroed."""
    _fields_ = [("lanes", C.c_int64), ("t", C.c_int32), ("num_steps", C.c_int32), ("recurrent_n", C.c_int32), ("hidden", C.c_int32),
                ("hidden_critic", C.c_int32), ("act_dim", C.c_int32), ("actions_int64", C.c_int32), ("reserved", C.c_int32),
                ("dones", C.c_void_p), ("values", C.c_void_p), ("actions_in", C.c_void_p), ("log_probs_in", C.c_void_p), ("rnn_in", C.c_void_p),
                ("rnn_critic_in", C.c_void_p), ("value_preds", C.c_void_p), ("actions", C.c_void_p), ("action_log_probs", C.c_void_p),
                ("rnn_states", C.c_void_p), ("rnn_states_critic", C.c_void_p), ("stride_dones", C.c_int64), ("stride_value_preds", C.c_int64),
                ("stride_actions", C.c_int64), ("stride_action_log_probs", C.c_int64), ("stride_rnn_states", C.c_int64),
                ("stride_rnn_states_critic", C.c_int64)]


class GmpeStepTailPlan(C.Structure):
    """gmpe_step_tail_plan (include/gmpe.h): gmpe_learner_plan with the step's masks, the stop rows of its position and the draw counter, one launch."""
    _fields_ = [("learner", GmpeLearnerPlan), ("num_agents", C.c_int32), ("n_actions", C.c_int32), ("masks", C.c_void_p), ("active_masks", C.c_void_p),
                ("available_actions", C.c_void_p), ("stride_masks", C.c_int64), ("stride_active_masks", C.c_int64),
                ("stride_available_actions", C.c_int64), ("draw_dev", C.c_void_p), ("draw_inc", C.c_uint64)]


class GmpeEpisodeRecordPlan(C.Structure):
    """gmpe_episode_record_plan (include/gmpe.h): one step of a batch of evaluation episodes, and the masks / stop rows for the next act."""
    _fields_ = [("num_envs", C.c_int32), ("num_agents", C.c_int32), ("t", C.c_int32), ("num_steps", C.c_int32), ("n_actions", C.c_int32),
                ("rnn_row", C.c_int32), ("reward", C.c_void_p), ("done", C.c_void_p), ("info", C.c_void_p), ("live", C.c_void_p),
                ("steps", C.c_void_p), ("ret", C.c_void_p), ("final_info", C.c_void_p), ("masks", C.c_void_p), ("available_actions", C.c_void_p),
                ("rnn_states", C.c_void_p)]


class GmpeEpisodeSeriesPlan(C.Structure):
    """gmpe_episode_series_plan (include/gmpe.h): one step of R back-to-back evaluation episodes per env; every env carries its own episode and step."""
    _fields_ = [("num_envs", C.c_int32), ("num_agents", C.c_int32), ("num_steps", C.c_int32), ("num_episodes", C.c_int32), ("n_actions", C.c_int32),
                ("rnn_row", C.c_int32), ("reward", C.c_void_p), ("done", C.c_void_p), ("info", C.c_void_p), ("episode", C.c_void_p),
                ("t_in_ep", C.c_void_p), ("ret", C.c_void_p), ("steps", C.c_void_p), ("ret_out", C.c_void_p), ("final_info", C.c_void_p),
                ("masks", C.c_void_p), ("available_actions", C.c_void_p), ("rnn_states", C.c_void_p)]


class GmpeEpisodeMetricsPlan(C.Structure):
    """gmpe_episode_metrics_plan (include/gmpe.h): the per-episode metric columns and the per-agent sums over episodes."""
    _fields_ = [("num_envs", C.c_int32), ("num_agents", C.c_int32), ("num_steps", C.c_int32), ("reserved", C.c_int32), ("dt", C.c_double),
                ("min_dist_thresh", C.c_double), ("steps", C.c_void_p), ("ret", C.c_void_p), ("final_info", C.c_void_p), ("episodes", C.c_void_p),
                ("dists_traveled", C.c_void_p), ("time_taken", C.c_void_p)]


class GmpeEpisodeSummaryPlan(C.Structure):
    """gmpe_episode_summary_plan (include/gmpe.h): min, p10, median, p90, max, mean, std of every column of an f64 table."""
    _fields_ = [("num_rows", C.c_int64), ("num_columns", C.c_int32), ("success_column", C.c_int32), ("success_agents", C.c_int32),
                ("reserved", C.c_int32), ("table", C.c_void_p), ("out", C.c_void_p)]


EVAL_INFO_WIDTH, EVAL_NUM_COLUMNS, EVAL_NUM_STATS = 18, 16, 7
INFOS_CHUNK, INFOS_LEAF = 8192, 128      # GMPE_INFOS_* of include/gmpe.h: NumPy's reduce buffer and pairwise_sum's block


class GmpeEnvInfosPlan(C.Structure):
    """gmpe_env_infos_plan (include/gmpe.h): np.mean over envs of every info column per agent, process_infos + log_env."""
    _fields_ = [("num_envs", C.c_int32), ("num_agents", C.c_int32), ("episode_length", C.c_int32), ("reserved", C.c_int32), ("dt", C.c_double),
                ("info", C.c_void_p), ("out", C.c_void_p)]


class GmpeEvalStepPlan(C.Structure):
    """gmpe_eval_step_plan (include/gmpe.h): one step of GMPERunner.eval's bookkeeping — reward sums, per-env masks, zeroed RNN rows."""
    _fields_ = [("num_envs", C.c_int32), ("num_agents", C.c_int32), ("rnn_row", C.c_int32), ("first", C.c_int32), ("reward", C.c_void_p),
                ("done", C.c_void_p), ("sums", C.c_void_p), ("masks", C.c_void_p), ("rnn_states", C.c_void_p)]


class GmpeEvalMeanPlan(C.Structure):
    """gmpe_eval_mean_plan (include/gmpe.h): np.mean of contiguous float64 values in NumPy's order."""
    _fields_ = [("count", C.c_int64), ("values", C.c_void_p), ("out", C.c_void_p)]


MB_FEED_FORWARD, MB_RECURRENT = 0, 1
MB_ROW, MB_ENV_ROW, MB_CHUNK_HEAD, MB_TABLE_NODE, MB_TABLE_ADJ = 0, 1, 2, 3, 4
MB_MAX_FIELDS = 20


class GmpeMbField(C.Structure):
    """gmpe_mb_field (include/gmpe.h): one field of a minibatch gather."""
    _fields_ = [("kind", C.c_int32), ("row_bytes", C.c_int32), ("slot_stride", C.c_int64), ("src", C.c_void_p), ("dst", C.c_void_p)]


class GmpeMinibatchPlan(C.Structure):
    """gmpe_minibatch_plan (include/gmpe.h): one PPO minibatch gathered from a rollout through a device permutation."""
    _fields_ = [("mode", C.c_int32), ("num_fields", C.c_int32), ("T", C.c_int32), ("N", C.c_int32), ("A", C.c_int32), ("L", C.c_int32),
                ("perm", C.c_void_p), ("perm_len", C.c_int64), ("offset", C.c_int64), ("rows", C.c_int64),
                ("fields", GmpeMbField * MB_MAX_FIELDS)]


MBE_ADJ, MBE_ADJ_COMPACT, MBE_TABLE = 0, 1, 2


class GmpeMbEdgesPlan(C.Structure):
    """gmpe_mb_edges_plan (include/gmpe.h): the edge list of one minibatch from the stored adjacency."""
    _fields_ = [("mode", C.c_int32), ("source", C.c_int32), ("T", C.c_int32), ("N", C.c_int32), ("A", C.c_int32), ("L", C.c_int32), ("E", C.c_int32),
                ("inclusive", C.c_int32), ("index64", C.c_int32), ("reuse_counts", C.c_int32), ("max_edge_dist", C.c_float), ("reserved", C.c_int32),
                ("perm", C.c_void_p), ("perm_len", C.c_int64), ("offset", C.c_int64), ("rows", C.c_int64), ("src", C.c_void_p), ("slot_stride", C.c_int64),
                ("edge_index", C.c_void_p), ("edge_attr", C.c_void_p), ("cap", C.c_int64), ("n_edges", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


PPO_POLICY_ACTIVE_MASKS, PPO_VALUE_ACTIVE_MASKS, PPO_CLIPPED_VALUE_LOSS, PPO_HUBER_LOSS, PPO_VALUENORM = 1, 2, 4, 8, 16
PPO_MAX_ACTIONS, PPO_NUM_OUT = 64, 7
PPO_OUT = ("policy_loss", "dist_entropy", "actor_loss", "value_loss", "ratio_mean", "denom_policy", "denom_value")


class GmpePpoLossPlan(C.Structure):
    """gmpe_ppo_loss_plan (include/gmpe.h): the loss arithmetic of one PPO minibatch with its gradients."""
    _fields_ = [("rows", C.c_int64), ("n_actions", C.c_int32), ("flags", C.c_int32), ("actions_int64", C.c_int32), ("reserved", C.c_int32),
                ("clip_param", C.c_double), ("huber_delta", C.c_double), ("entropy_coef", C.c_double), ("beta", C.c_double), ("epsilon", C.c_double),
                ("logits", C.c_void_p), ("values", C.c_void_p), ("actions", C.c_void_p), ("available_actions", C.c_void_p),
                ("old_action_log_probs", C.c_void_p), ("adv_targ", C.c_void_p), ("value_preds", C.c_void_p), ("returns", C.c_void_p),
                ("active_masks", C.c_void_p), ("running_mean", C.c_void_p), ("running_mean_sq", C.c_void_p), ("debiasing_term", C.c_void_p),
                ("out", C.c_void_p), ("grad_logits", C.c_void_p), ("grad_values", C.c_void_p), ("action_log_probs", C.c_void_p),
                ("imp_weights", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class GmpePpoLossShardPlan(C.Structure):
    """gmpe_ppo_loss_shard_plan (include/gmpe.h): gmpe_ppo_loss_plan in two phases around an exchange of the shards' sums and row counts."""
    _fields_ = [("base", GmpePpoLossPlan), ("phase", C.c_int32), ("world", C.c_int32), ("local", C.c_void_p), ("all", C.c_void_p)]


POPART_MAX_HIDDEN = 1024


class GmpePopartLossPlan(C.Structure):
    """gmpe_popart_loss_plan (include/gmpe.h): the same minibatch with PopArt, from the critic's features to the rescaled output layer."""
    _fields_ = [("rows", C.c_int64), ("n_actions", C.c_int32), ("hidden", C.c_int32), ("flags", C.c_int32), ("actions_int64", C.c_int32),
                ("clip_param", C.c_double), ("huber_delta", C.c_double), ("entropy_coef", C.c_double), ("beta", C.c_double), ("epsilon", C.c_double),
                ("logits", C.c_void_p), ("critic_features", C.c_void_p), ("actions", C.c_void_p), ("available_actions", C.c_void_p),
                ("old_action_log_probs", C.c_void_p), ("adv_targ", C.c_void_p), ("value_preds", C.c_void_p), ("returns", C.c_void_p),
                ("active_masks", C.c_void_p), ("weight", C.c_void_p), ("bias", C.c_void_p), ("stddev", C.c_void_p), ("mean", C.c_void_p),
                ("mean_sq", C.c_void_p), ("debiasing_term", C.c_void_p), ("weight_out", C.c_void_p), ("bias_out", C.c_void_p),
                ("stddev_out", C.c_void_p), ("values_out", C.c_void_p), ("out", C.c_void_p), ("grad_logits", C.c_void_p),
                ("grad_features", C.c_void_p), ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p), ("action_log_probs", C.c_void_p),
                ("imp_weights", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class GmpeActPlan(C.Structure):
    """gmpe_act_plan (include/gmpe.h): the rollout half of the action head — one action and its log-prob per row of logits."""
    _fields_ = [("rows", C.c_int64), ("n_actions", C.c_int32), ("num_agents", C.c_int32), ("stop_action", C.c_int32), ("deterministic", C.c_int32),
                ("env_id_base", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("draw", C.c_uint64), ("draw_inc", C.c_uint64),
                ("draw_dev", C.c_void_p), ("logits", C.c_void_p), ("available_actions", C.c_void_p), ("dones_prev", C.c_void_p),
                ("action_idx", C.c_void_p), ("log_probs", C.c_void_p), ("actions_f32", C.c_void_p), ("actions_i64", C.c_void_p)]


class GmpeHeadPlan(C.Structure):
    """gmpe_head_plan (include/gmpe.h): the Linear of the policy's action head, forward, backward and inside the rollout's sampling launch."""
    _fields_ = [("rows", C.c_int64), ("n_actions", C.c_int32), ("hidden", C.c_int32), ("features", C.c_void_p), ("weight", C.c_void_p),
                ("bias", C.c_void_p), ("logits_out", C.c_void_p), ("grad_logits", C.c_void_p), ("grad_features", C.c_void_p),
                ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class GmpeValuePlan(C.Structure):
    """gmpe_value_plan (include/gmpe.h): the critic's value head v_out, forward and backward."""
    _fields_ = [("rows", C.c_int64), ("hidden", C.c_int32), ("reserved", C.c_int32), ("features", C.c_void_p), ("weight", C.c_void_p),
                ("bias", C.c_void_p), ("values_out", C.c_void_p), ("grad_values", C.c_void_p), ("grad_features", C.c_void_p),
                ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


GRU_ROW_TILE = 32        # GMPE_GRU_ROW_TILE of include/gmpe.h; tests/gru_lib.py TILE is the third copy — tests/test_abi_host.py compiles against the header, tests/test_gru_host.py ties the three together


class GmpeGruPlan(C.Structure):
    """gmpe_gru_plan (include/gmpe.h): the policy's masked GRU layer with its LayerNorm, forward and backward."""
    _fields_ = [("steps", C.c_int64), ("rows", C.c_int64), ("in_dim", C.c_int32), ("hidden", C.c_int32), ("eps", C.c_double),
                ("x", C.c_void_p), ("hxs", C.c_void_p), ("masks", C.c_void_p), ("weight_ih", C.c_void_p), ("weight_hh", C.c_void_p),
                ("bias_ih", C.c_void_p), ("bias_hh", C.c_void_p), ("ln_weight", C.c_void_p), ("ln_bias", C.c_void_p), ("features", C.c_void_p),
                ("hxs_out", C.c_void_p), ("grad_features", C.c_void_p), ("grad_hxs_out", C.c_void_p), ("grad_x", C.c_void_p), ("grad_hxs", C.c_void_p),
                ("grad_weight_ih", C.c_void_p), ("grad_weight_hh", C.c_void_p), ("grad_bias_ih", C.c_void_p), ("grad_bias_hh", C.c_void_p),
                ("grad_ln_weight", C.c_void_p), ("grad_ln_bias", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


MLP_ROW_TILE, MLP_MAX_PARTS, MLP_MAX_IN, MLP_MAX_LAYERS = 32, 4, 256, 3      # GMPE_MLP_* of include/gmpe.h; tests/test_abi_host.py compiles against the header
MLP_RELU, MLP_TANH = 0, 1


class GmpeMlpLayer(C.Structure):
    """gmpe_mlp_layer (include/gmpe.h): one Linear -> activation -> LayerNorm of the MLPBase, with its gradients."""
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("ln_weight", C.c_void_p), ("ln_bias", C.c_void_p), ("eps", C.c_double),
                ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p), ("grad_ln_weight", C.c_void_p), ("grad_ln_bias", C.c_void_p)]


class GmpeMlpPlan(C.Structure):
    """gmpe_mlp_plan (include/gmpe.h): the policy's MLPBase over the parts of its input, forward and backward."""
    _fields_ = [("rows", C.c_int64), ("hidden", C.c_int32), ("layer_n", C.c_int32), ("activation", C.c_int32), ("feature_norm", C.c_int32),
                ("n_parts", C.c_int32), ("reserved", C.c_int32), ("part", C.c_void_p * MLP_MAX_PARTS), ("part_dim", C.c_int32 * MLP_MAX_PARTS),
                ("grad_part", C.c_void_p * MLP_MAX_PARTS), ("fn_weight", C.c_void_p), ("fn_bias", C.c_void_p), ("fn_eps", C.c_double),
                ("grad_fn_weight", C.c_void_p), ("grad_fn_bias", C.c_void_p), ("layer", GmpeMlpLayer * MLP_MAX_LAYERS), ("features", C.c_void_p),
                ("grad_features", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


# GMPE_GNN_* of include/gmpe.h; tests/test_abi_host.py compiles against the header
GNN_HIDDEN, GNN_MAX_NODES, GNN_MAX_HEADS, GNN_MAX_CONVS, GNN_MAX_EMBED_LAYERS = 16, 64, 4, 3, 2
GNN_MAX_FEATS, GNN_MAX_EMBEDDINGS, GNN_MAX_EMBEDDING_SIZE = 16, 16, 8
GNN_WIDE_MAX_NODES = 128                # the forward-only entries gmpe_gnn_forward_wide / _wide_table
GNN_RELU, GNN_TANH = 0, 1
GNN_NODE, GNN_MEAN, GNN_MAX, GNN_ADD = 0, 1, 2, 3
GNN_CONV_PARAMS = ("query_weight", "query_bias", "key_weight", "key_bias", "value_weight", "value_bias", "edge_weight", "skip_weight", "skip_bias")


class GmpeGnnConv(C.Structure):
    """gmpe_gnn_conv (include/gmpe.h): one TransformerConv of the GNNBase, with its gradients."""
    _fields_ = [(k, C.c_void_p) for k in GNN_CONV_PARAMS] + [("grad_" + k, C.c_void_p) for k in GNN_CONV_PARAMS]


class GmpeGnnPlan(C.Structure):
    """gmpe_gnn_plan (include/gmpe.h): the policy's GNNBase from the dense adjacency, forward and backward."""
    _fields_ = [("rows", C.c_int64)] + [(k, C.c_int32) for k in (
        "num_nodes", "node_feats", "adj_share", "hidden", "heads", "concat", "beta", "edge_dim", "gnn_layer_n", "embed_layer_n", "embed_activation",
        "conv_activation", "embed_layer_norm", "aggregate", "num_embeddings", "embedding_size")] + [
        ("max_edge_dist", C.c_double), ("ln_eps", C.c_double), ("node_obs", C.c_void_p), ("adj", C.c_void_p), ("agent_id", C.c_void_p),
        ("entity_embed", C.c_void_p), ("lin1_weight", C.c_void_p), ("lin1_bias", C.c_void_p), ("ln_weight", C.c_void_p), ("ln_bias", C.c_void_p),
        ("embed_weight", C.c_void_p * GNN_MAX_EMBED_LAYERS), ("embed_bias", C.c_void_p * GNN_MAX_EMBED_LAYERS),
        ("grad_entity_embed", C.c_void_p), ("grad_lin1_weight", C.c_void_p), ("grad_lin1_bias", C.c_void_p), ("grad_ln_weight", C.c_void_p),
        ("grad_ln_bias", C.c_void_p), ("grad_embed_weight", C.c_void_p * GNN_MAX_EMBED_LAYERS), ("grad_embed_bias", C.c_void_p * GNN_MAX_EMBED_LAYERS),
        ("conv", GmpeGnnConv * GNN_MAX_CONVS), ("features", C.c_void_p), ("grad_features", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t)]


class GmpeGnnTablePlan(C.Structure):
    """gmpe_gnn_table_plan (include/gmpe.h): the same GNNBase with a graph's rows and matrix rebuilt from an fp64 entity table."""
    _fields_ = [("base", GmpeGnnPlan), ("cfg", C.POINTER(GmpeConfig)), ("table", C.c_void_p), ("table_rows", C.c_int64),
                ("table_index", C.c_void_p), ("index64", C.c_int32), ("table_share", C.c_int32)]


# GMPE_OPT_* of include/gmpe.h; tests/test_abi_host.py compiles against the header
OPT_MAX_TENSORS, OPT_MAX_HYPERS, OPT_CHUNK, OPT_MAX_PLAN_TENSORS, OPT_MAX_NUMEL = 64, 8, 1024, 4096, 1 << 30
OPT_CLIP, OPT_STEP = 1, 2
OPT_T_IN_NORM, OPT_T_STEP = 1, 2
OPT_HYPER_FLOATS, OPT_MAX_SCHEDULE_ROWS = 7, 1 << 20


class GmpeOptimTensor(C.Structure):
    """gmpe_optim_tensor (include/gmpe.h): one tensor of the clip-and-step table."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64),
                ("flags", C.c_int32), ("hyper", C.c_int32)]


class GmpeOptimHyper(C.Structure):
    """gmpe_optim_hyper (include/gmpe.h): one torch param_group at one step count."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double), ("t", C.c_int64)]


class GmpeOptimPlan(C.Structure):
    """gmpe_optim_plan (include/gmpe.h): clip_grad_norm_ and Adam.step over a table of tensors."""
    _fields_ = [("n_tensors", C.c_int32), ("n_hypers", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("tensors", C.POINTER(GmpeOptimTensor)), ("hypers", C.POINTER(GmpeOptimHyper)), ("max_norm", C.c_double), ("out", C.c_void_p),
                ("grad_norm_f32", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class GmpeOptimShardPlan(C.Structure):
    """gmpe_optim_shard_plan (include/gmpe.h): gmpe_optim_plan in two phases around an all-gather of the shards' packed gradients."""
    _fields_ = [("base", GmpeOptimPlan), ("phase", C.c_int32), ("world", C.c_int32), ("local", C.c_void_p), ("all", C.c_void_p),
                ("local_elems", C.c_int64)]


class GmpeOptimSchedPlan(C.Structure):
    """gmpe_optim_sched_plan (include/gmpe.h): gmpe_optim_plan with Adam's step count on the device — the Hyper sets of `rows` steps and a counter."""
    _fields_ = [("base", GmpeOptimPlan), ("schedule", C.c_void_p), ("counter", C.c_void_p), ("status", C.c_void_p), ("rows", C.c_int32),
                ("reserved", C.c_int32)]


class GmpeError(RuntimeError):
    pass


def load():
    """Load libgmpe.so. torch must be imported first so that the engine binds to the SAME HIP
    runtime (libamdhip64.so.7) torch uses; two runtimes in one process cannot share device memory."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GmpeError("libgmpe.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "or `make -C contracts-marl-aam-corridors_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    import torch  # noqa: F401  (loads libamdhip64 first)
    lib = C.CDLL(LIB_PATH)
    P, I = C.c_void_p, C.c_int
    lib.gmpe_last_error.restype = C.c_char_p
    lib.gmpe_obs_dim.argtypes = [C.POINTER(GmpeConfig)]
    lib.gmpe_node_feats.argtypes = [C.POINTER(GmpeConfig)]
    lib.gmpe_num_entities.argtypes = [C.POINTER(GmpeConfig)]
    lib.gmpe_create.argtypes = [C.POINTER(GmpeConfig), I, C.POINTER(P)]
    lib.gmpe_destroy.argtypes = [P]
    lib.gmpe_set_rng_tape.argtypes = [P, P, C.c_int64]
    lib.gmpe_reset.argtypes = [P, P, C.POINTER(GmpeOutputs), P]
    lib.gmpe_step.argtypes = [P, P, C.POINTER(GmpeOutputs), P]
    lib.gmpe_step_envs.argtypes = [P, P, C.POINTER(GmpeOutputs), C.c_int32, C.c_int32, P]
    lib.gmpe_step_many_envs.argtypes = [P, P, C.c_int32, C.c_int32, C.POINTER(GmpeOutputs), C.c_int32, P]
    lib.gmpe_step_onehot.argtypes = [P, P, C.POINTER(GmpeOutputs), P]
    lib.gmpe_step_many.argtypes = [P, P, C.c_int32, C.c_int32, C.POINTER(GmpeOutputs), P]
    lib.gmpe_step_many_launches.argtypes = [P, P, C.c_int32, C.c_int32, C.POINTER(GmpeOutputs), P]
    lib.gmpe_step_many_prepare.argtypes = [P, P, C.c_int32, C.c_int32, C.POINTER(GmpeOutputs)]
    lib.gmpe_field_bytes.argtypes = [P, I, C.POINTER(C.c_size_t)]
    lib.gmpe_get_field.argtypes = [P, I, P, C.c_size_t]
    lib.gmpe_set_field.argtypes = [P, I, P, C.c_size_t]
    lib.gmpe_edges_from_adj.argtypes = [P, P, C.c_int32, C.c_int32, C.c_float, C.c_int32, P, P, C.c_int32, P, P]
    lib.gmpe_edges_from_adj_compact.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, P, P, C.c_int64, P, P]
    lib.gmpe_masks_from_dones.argtypes = [P, P, P, P, P]
    lib.gmpe_set_control_override.argtypes = [P, P, P]
    lib.gmpe_field_device_ptr.argtypes = [P, I, C.POINTER(P)]
    lib.gmpe_timing_enable.argtypes = [P, C.c_int32]
    lib.gmpe_timing_read.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]
    lib.gmpe_timing_mark.argtypes = [P, C.c_int32, P]
    lib.gmpe_timing_region_ms.argtypes = [P, C.POINTER(C.c_double)]
    lib.gmpe_rollout_steps.argtypes = [P, P, C.POINTER(GmpeRollout), C.POINTER(GmpeOutputs), P]
    lib.gmpe_get_tuning.argtypes = [P, C.POINTER(GmpeTuning)]
    lib.gmpe_entity_table_width.argtypes = [C.POINTER(GmpeConfig)]
    lib.gmpe_expand_node_obs.argtypes = [C.POINTER(GmpeConfig), I, P, C.c_int64, C.c_int64, P, C.c_int64, C.c_int64, P]
    lib.gmpe_expand_adj.argtypes = [C.POINTER(GmpeConfig), I, P, C.c_int64, C.c_int64, P, C.c_int64, C.c_int64, C.c_int32, P]
    lib.gmpe_returns_workspace_bytes.argtypes = [C.c_int64, C.POINTER(C.c_size_t)]
    lib.gmpe_compute_returns.argtypes = [I, C.POINTER(GmpeReturnsPlan), P]
    lib.gmpe_available_actions_from_dones.argtypes = [I, C.POINTER(GmpeAvailPlan), P]
    lib.gmpe_minibatch_gather.argtypes = [C.POINTER(GmpeConfig), I, C.POINTER(GmpeMinibatchPlan), P]
    lib.gmpe_minibatch_edges.argtypes = [C.POINTER(GmpeConfig), I, C.POINTER(GmpeMbEdgesPlan), P]
    lib.gmpe_minibatch_edges_workspace_bytes.argtypes = [C.c_int64, C.POINTER(C.c_size_t)]
    lib.gmpe_insert_learner.argtypes = [I, C.POINTER(GmpeLearnerPlan), P]
    lib.gmpe_step_tail.argtypes = [I, C.POINTER(GmpeStepTailPlan), P]
    lib.gmpe_episode_record.argtypes = [I, C.POINTER(GmpeEpisodeRecordPlan), P]
    lib.gmpe_episode_record_series.argtypes = [I, C.POINTER(GmpeEpisodeSeriesPlan), P]
    lib.gmpe_episode_metrics.argtypes = [I, C.POINTER(GmpeEpisodeMetricsPlan), P]
    lib.gmpe_episode_summary.argtypes = [I, C.POINTER(GmpeEpisodeSummaryPlan), P]
    lib.gmpe_ppo_loss.argtypes = [I, C.POINTER(GmpePpoLossPlan), P]
    lib.gmpe_ppo_loss_workspace_bytes.argtypes = [C.c_int64, C.POINTER(C.c_size_t)]
    lib.gmpe_ppo_loss_popart.argtypes = [I, C.POINTER(GmpePopartLossPlan), P]
    lib.gmpe_ppo_loss_popart_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]
    lib.gmpe_act_sample.argtypes = [I, C.POINTER(GmpeActPlan), P]
    lib.gmpe_compute_returns_shard.argtypes = [I, C.POINTER(GmpeReturnsShardPlan), P]
    lib.gmpe_ppo_loss_shard.argtypes = [I, C.POINTER(GmpePpoLossShardPlan), P]
    lib.gmpe_gru_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]
    lib.gmpe_gru_forward.argtypes = [I, C.POINTER(GmpeGruPlan), P]
    lib.gmpe_gru_backward.argtypes = [I, C.POINTER(GmpeGruPlan), P]
    lib.gmpe_mlp_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]
    lib.gmpe_mlp_forward.argtypes = [I, C.POINTER(GmpeMlpPlan), P]
    lib.gmpe_mlp_backward.argtypes = [I, C.POINTER(GmpeMlpPlan), P]
    lib.gmpe_gnn_workspace_bytes.argtypes = [C.POINTER(GmpeGnnPlan), C.c_int32, C.POINTER(C.c_size_t)]
    lib.gmpe_gnn_forward.argtypes = [I, C.POINTER(GmpeGnnPlan), P]
    lib.gmpe_gnn_backward.argtypes = [I, C.POINTER(GmpeGnnPlan), P]
    lib.gmpe_gnn_forward_table.argtypes = [I, C.POINTER(GmpeGnnTablePlan), P]
    lib.gmpe_gnn_backward_table.argtypes = [I, C.POINTER(GmpeGnnTablePlan), P]
    lib.gmpe_gnn_forward_wide.argtypes = [I, C.POINTER(GmpeGnnPlan), P]
    lib.gmpe_gnn_forward_wide_table.argtypes = [I, C.POINTER(GmpeGnnTablePlan), P]
    lib.gmpe_gnn_wide_geometry.argtypes = [C.POINTER(GmpeGnnPlan), C.POINTER(C.c_int64)]
    lib.gmpe_head_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]
    lib.gmpe_head_forward.argtypes = [I, C.POINTER(GmpeHeadPlan), P]
    lib.gmpe_head_backward.argtypes = [I, C.POINTER(GmpeHeadPlan), P]
    lib.gmpe_act_head.argtypes = [I, C.POINTER(GmpeActPlan), C.POINTER(GmpeHeadPlan), P]
    lib.gmpe_value_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]
    lib.gmpe_value_forward.argtypes = [I, C.POINTER(GmpeValuePlan), P]
    lib.gmpe_value_backward.argtypes = [I, C.POINTER(GmpeValuePlan), P]
    lib.gmpe_optim_workspace_bytes.argtypes = [C.POINTER(GmpeOptimPlan), C.POINTER(C.c_size_t)]
    lib.gmpe_optim_step.argtypes = [I, C.POINTER(GmpeOptimPlan), P]
    lib.gmpe_optim_shard_elems.argtypes = [C.POINTER(GmpeOptimPlan), C.POINTER(C.c_int64)]
    lib.gmpe_optim_step_shard.argtypes = [I, C.POINTER(GmpeOptimShardPlan), P]
    lib.gmpe_optim_schedule_bytes.argtypes = [C.POINTER(GmpeOptimPlan), C.c_int32, C.POINTER(C.c_size_t)]
    lib.gmpe_optim_schedule_fill.argtypes = [C.POINTER(GmpeOptimPlan), C.c_int32, P]
    lib.gmpe_optim_step_scheduled.argtypes = [I, C.POINTER(GmpeOptimSchedPlan), P]
    lib.gmpe_env_infos.argtypes = [I, C.POINTER(GmpeEnvInfosPlan), P]
    lib.gmpe_eval_step.argtypes = [I, C.POINTER(GmpeEvalStepPlan), P]
    lib.gmpe_eval_mean.argtypes = [I, C.POINTER(GmpeEvalMeanPlan), P]
    from .config import ABI_VERSION
    if lib.gmpe_abi_version() != ABI_VERSION:
        raise GmpeError("libgmpe.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise GmpeError("%s failed (%d): %s" % (what, rc, load().gmpe_last_error().decode()))
