/* gmpe.h — C ABI of the MI355X batched GraphMPE step engine (libgmpe.so).
 *
 * This is the drop-in boundary for ONE hot path of Jaroan/Contracts-MARL-AAM-Corridors: the
 * per-environment particle-world step + graph observation, batched over N environments.
 * It replaces what `GraphSubprocVecEnv` (onpolicy/envs/env_wrappers.py:959-1037) obtains from its
 * N worker processes, each of which runs `MultiAgentGraphEnv.step/reset`
 * (multiagent/environment.py:1021-1081) on `World.step` (multiagent/core.py:687-756) with the
 * scenario callbacks of multiagent/custom_scenarios/nav_metered_one_goal_graph_rotate_tube_july.py.
 *
 * Conventions
 *  - plain C: POD structs, raw pointers, sizes. No torch / C++ types cross this boundary.
 *  - every function returns 0 on success or a negative gmpe_status; gmpe_last_error() gives text.
 *    No exception crosses the ABI.
 *  - "dev" pointers are device (HBM) pointers owned by the CALLER (e.g. torch tensors'
 *    data_ptr()); "host" pointers are ordinary host memory. The handle owns only the persistent
 *    SoA world state and scratch (a few KB; plus one [N,E,E] float matrix for handles on the split
 *    big-E path, allocated by gmpe_create); step/reset never allocate.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream). step/reset are
 *    asynchronous on it; get/set_field synchronise the handle's stream themselves.
 *  - one handle per GPU; handles are not thread-safe.
 *
 * Shapes: N envs, A agents, L landmarks, O obstacles, E = A+L+O graph nodes, F = 8 node features,
 * D = observation width (19 tube_july, 13 navigation_graph, 13 rot_inv); F = 8 (7 for rot_inv and for graph_feat_type 'global').
 */
#ifndef GMPE_H
#define GMPE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMPE_ABI_VERSION 3
#define GMPE_NODE_FEATS 8          /* …_july.py:1771  [rel_vel2, rel_pos2, rel_goal2, occupied, type]; rot_inv: 7 (gmpe_node_feats) */
#define GMPE_INFO_KEYS 18          /* …_july.py:806-828 + 'individual_reward' (environment.py:1048) + 'Phase_reached' (rot_inv:835) */
#define GMPE_MAX_AGENTS 64         /* one wavefront lane per agent in the sequential-semantics pass   */
#define GMPE_MAX_ENTITIES 160
#define GMPE_MAX_WALLS 8
#define GMPE_TUBE_STRIDE 12

typedef enum gmpe_status {
    GMPE_OK = 0,
    GMPE_ERR_INVALID_ARG = -1,
    GMPE_ERR_HIP = -2,              /* a HIP runtime call failed (text in gmpe_last_error)            */
    GMPE_ERR_NO_DEVICE = -3,
    GMPE_ERR_UNSUPPORTED = -4,
    GMPE_ERR_TAPE_EXHAUSTED = -5,   /* parity mode: an env needed more uniform draws than the tape has */
    GMPE_ERR_PLACEMENT = -6         /* reset: rejection sampler hit GMPE_MAX_PLACEMENT_TRIES           */
} gmpe_status;

/* Scenarios (multiagent/custom_scenarios/<name>.py). */
typedef enum gmpe_scenario {
    GMPE_SCENARIO_NAVIGATION_GRAPH = 0, /* not shipped by the reference (train_mpe.py:72-73 default only):
                                           restated from extant blocks, see DESIGN.md §navigation_graph */
    GMPE_SCENARIO_TUBE_JULY = 1,        /* nav_metered_one_goal_graph_rotate_tube_july.py               */
    GMPE_SCENARIO_ROT_INV = 2,          /* nav_graph_metered_single_corridor_rot_inv.py: rotation-
                                           invariant 13-d obs, 7 node features, exit gate + progress reward, armed cooldown */
    GMPE_SCENARIO_TWO_PHASE = 3,        /* two_phase_graph.py: rot_inv family, 15-d obs (exit vector, heading alignment), random
                                           tube length, episode ends for an agent at the exit gate, no collision reward term  */
    GMPE_SCENARIO_THREE_PHASE = 4       /* three_phase_graph.py: two_phase + post-tube goal phase, -collision_rew per contact   */
} gmpe_scenario;

/* Dynamics (multiagent/core.py:23-26 EntityDynamicsType). */
typedef enum gmpe_dynamics {
    GMPE_DYN_DOUBLE_INTEGRATOR = 0,     /* force path: core.py:766-845, 872-964                       */
    GMPE_DYN_UNICYCLE = 1,              /* kinematic, UnicycleVehicleConfig constants                 */
    GMPE_DYN_AIR_TAXI = 2               /* kinematic: core.py:231-340, 819-826                        */
} gmpe_dynamics;

/* args.formation_type (…_july.py:192, 492-497): where random_scenario puts the landmarks (goal i belongs to agent i). */
typedef enum gmpe_formation {
    GMPE_FORMATION_POINT = 0,           /* set_landmarks_in_point (custom_scenarios/utils.py:165-193): all at exit + R(angle) @ [0, -ws/3]      */
    GMPE_FORMATION_LINE = 1,            /* set_landmarks_in_line (utils.py:77-130) called with start (-ws/2, -ws/2), end (ws/2, -ws/2):
                                           np.linspace(start, end, L) — the zero y-step takes linspace's (i / div) * delta branch             */
    GMPE_FORMATION_CIRCLE = 2           /* set_landmarks_in_circle (utils.py:231-267): centre (0, exit_y + ws/5), radius ws/3, angle i * 2 pi / L */
} gmpe_formation;

typedef struct gmpe_wall {              /* multiagent/core.py:354-373 Wall                             */
    int32_t orient;                     /* 0 = 'H' (lies along x at y = axis_pos), 1 = 'V'            */
    int32_t hard;
    double axis_pos;
    double end0, end1;
    double width;
} gmpe_wall;

/* Everything the reference reads from `args` (…_july.py:155-192,206-224,248-259,274,315,326) and
 * from multiagent/config.py, frozen into one POD. The Python host fills it (gmpe/config.py). */
typedef struct gmpe_config {
    int32_t abi_version;                /* GMPE_ABI_VERSION                                            */
    int32_t scenario;                   /* gmpe_scenario                                               */
    int32_t dynamics;                   /* gmpe_dynamics                                               */
    int32_t num_envs;                   /* N on this handle                                            */
    int32_t num_agents;                 /* A  (== num_landmarks: goal i belongs to agent i, :356)      */
    int32_t num_landmarks;              /* L                                                           */
    int32_t num_obstacles;              /* O                                                           */
    int32_t num_walls;                  /* physics only, never graph nodes                             */
    int32_t episode_length;             /* world.world_length (environment.py:264-271)                 */
    int32_t env_id_base;                /* global id of env 0 of this handle: RNG key = seed, id       */
    int32_t n_actions;                  /* 25 (5x5 motion primitives) or 5 / 9 (double integrator)     */
    int32_t collaborative;              /* shared reward (environment.py:1056-1061)                    */
    uint64_t seed;
    double world_size;
    double max_speed;                   /* args.max_speed (agent.max_speed; <=0 means None)            */
    double collision_rew, formation_rew, goal_rew;
    double min_reward, max_reward;      /* RewardWeightConfig.MIN/MAX_REWARD (config.py:135-136)       */
    /* multiagent/config.py constants of the chosen dynamics */
    double dt;
    double v_min, v_max;                /* kinematic speed clamp (core.py:309-312); DI: v_max = VX_MAX */
    double goal_thresh;                 /* DISTANCE_TO_GOAL_THRESHOLD                                  */
    double sep_dist;                    /* COLLISION_DISTANCE (= SEPARATION_DISTANCE for air_taxi)     */
    double coord_range;                 /* COORDINATION_RANGE: update_graph max_edge_dist (:242)       */
    double ang_rate_opt[5];             /* np.linspace(-ANGULAR_RATE_MAX, +, 5) (environment.py:441)   */
    double accel_opt[5];                /* np.linspace(ACCEL_MIN, ACCEL_MAX, 5)   (environment.py:440) */
    double sensitivity;                 /* 5.0 (environment.py:460-463)                                */
    double entity_size;                 /* Entity.size = 0.06 (core.py:385)                            */
    /* force path (core.py:542-548) */
    double damping, contact_force, contact_margin, wall_contact_force, wall_contact_margin;
    gmpe_wall walls[GMPE_MAX_WALLS];
    /* ---- ABI 2 ---- */
    int32_t graph_feat_type;            /* 0 'relative' (…_july.py:1694-1771, F = 8; rot_inv family F = 7); 1 'global' (…_july.py:1672-1691,
                                           rot_inv.py:1668-1687: [vel, pos, goal, type] in world coordinates, F = 7, every scenario)  */
    int32_t contact_family;             /* force path constants: 0 = multiagent/core.py:872-906 (d_min = COLLISION_DISTANCE, no force on a
                                           done side, separate wall constants); 1 = classic MPE, onpolicy/envs/mpe/core.py:273-286
                                           (d_min = size_a + size_b, every collider side gets its force, walls share the contact
                                           constants). navigation_graph only                                                      */
    double agent_size, collider_size;   /* classic: Entity.size of agents / of obstacles (mpe/core.py:44)                          */
    double agent_mass;                  /* Entity.mass (mpe/core.py:52 initial_mass = 1.0): v += F / mass * dt                     */
    double action_force_scale;          /* apply_action_force (mpe/core.py:205-214): mass * accel if accel is not None else mass   */
    /* ---- ABI 3 ---- */
    int32_t formation_type;             /* gmpe_formation: landmark placement of the tube scenarios' reset (…_july.py:492-497, rot_inv.py:493-498,
                                           two_phase_graph.py:464-469, three_phase_graph.py:459-464); navigation_graph does not read it        */
    int32_t reserved0;
} gmpe_config;

/* Persistent per-env state, addressable for checkpoint / parity injection. */
typedef enum gmpe_field {
    GMPE_F_X = 0,            /* f64 [N,A]                                                               */
    GMPE_F_Y,                /* f64 [N,A]                                                               */
    GMPE_F_S2,               /* f64 [N,A]  air_taxi/unicycle: theta        double_integrator: v_x       */
    GMPE_F_S3,               /* f64 [N,A]  air_taxi/unicycle: speed        double_integrator: v_y       */
    GMPE_F_P_DIST,           /* f64 [N,A]  odometer (core.py:315)                                       */
    GMPE_F_TIME,             /* f64 [N,A]  (core.py:316)                                                */
    GMPE_F_STATUS,           /* u8  [N,A]  agent.status (done)                                          */
    GMPE_F_PREV_PHASE,       /* i32 [N,A]  agent.previous_phase — survives resets (…_july.py:708-710)   */
    GMPE_F_PHASE_REACHED,    /* i32 [N,A]                                                               */
    GMPE_F_COOLDOWN,         /* i32 [N,A]  entry_reward_cooldown (never armed in the July file)         */
    GMPE_F_GOAL_TRACKER,     /* i32 [N,A]                                                               */
    GMPE_F_CURRENT_STEP,     /* i32 [N]                                                                 */
    GMPE_F_RNG_CTR,          /* i64 [N]    uniform draws consumed so far by this env                    */
    GMPE_F_TUBE,             /* f64 [N,12] angle, ent.xy, exit.xy, e.xy, n.xy(fp32-rounded), L, half_w, width */
    GMPE_F_LANDMARKS,        /* f64 [N,L,2]                                                             */
    GMPE_F_OBSTACLES,        /* f64 [N,O,2]                                                             */
    /* info counters (…_july.py:741-829); the int-typed ones reproduce the reference's np.full(n,-1)
       int64 arrays, into which floats are truncated on assignment */
    GMPE_F_TIMES_REQUIRED,   /* i32 [N,A] */
    GMPE_F_DISTS_TO_GOAL,    /* i32 [N,A] */
    GMPE_F_DIST_LEFT,        /* i32 [N,A] */
    GMPE_F_GOAL_REACHED,     /* i32 [N,A] */
    GMPE_F_N_AGENT_COLL,     /* i32 [N,A] */
    GMPE_F_N_OBST_COLL,      /* i32 [N,A] */
    GMPE_F_SPACING_VIOL,     /* i32 [N,A] */
    GMPE_F_STEPS_IN_CORR,    /* i32 [N,A] */
    GMPE_F_CONFORMANCE,      /* i32 [N,A] */
    GMPE_F_GOAL_MIN_TIME,    /* f64 [N,A] agent.goal_min_time (…_july.py:941-951)                       */
    GMPE_F_DELTA_SPACING,    /* f64 [N]   running sum of the delta_spacing list (:1180, :802)           */
    GMPE_F_ERROR_FLAGS,      /* i32 [N]   sticky: bit0 tape exhausted, bit1 placement gave up           */
    GMPE_F_PREV_PROJ,        /* f64 [N,A] rot_inv: prev_proj (a float32 array in the reference, :374, 1268-1276) */
    GMPE_F_COUNT
} gmpe_field;

typedef struct gmpe_handle gmpe_handle;

/* Output buffers of one step/reset, all caller-owned DEVICE memory. Any pointer may be NULL to
 * skip that output. Layout = what GraphSubprocVecEnv.step_wait stacks (env_wrappers.py:996-1004),
 * narrowed to the dtypes GraphReplayBuffer stores (onpolicy/utils/graph_buffer.py:84-114). */
typedef struct gmpe_outputs {
    float*   obs;        /* [N,A,D]                                                                    */
    int32_t* agent_id;   /* [N,A,1]                    (…_july.py:1554-1555)                           */
    float*   node_obs;   /* [N,A,E,F]  F = gmpe_node_feats (…_july.py:1584-1624, 1694-1771)            */
    float*   adj;        /* adj_compact ? [N,E,E] : [N,A,E,E]  (…_july.py:1625-1648)                   */
    float*   reward;     /* [N,A]   (step only)        (…_july.py:1105-1221)                           */
    uint8_t* done;       /* [N,A]   (step only)        (environment.py:264-271)                        */
    float*   info;       /* [N,A,GMPE_INFO_KEYS] (step only; optional) (…_july.py:741-829)             */
    int32_t  adj_compact;/* 1: write the single E×E matrix every ego shares            */
    int32_t  reserved;
    /* ---- ABI 3 ---- */
    double*  entity_table;/* [N,W] f64, W = gmpe_entity_table_width(cfg), or NULL: the per-entity state the node_obs rows of this step are a pure function of —
                            what a rank SHIPS instead of the [N,A,E,F] rows (SURVEY §8e "state + one E×E per env"); gmpe_expand_node_obs rebuilds the rows
                            bit for bit on the learner. Layout per env: x[E], y[E] of every entity (agents after the move / after a reset), then per agent
                            vox[A], voy[A] (velocity BEFORE this step's reward loop), vnx[A], vny[A] (AFTER it: re-drawn heading on a goal reach, core.py:324-333);
                            rot_inv family: + cos[A], sin[A] of the post-reward heading; two_phase_graph: + exit x, exit y (its goal node feature); last, ceil(E / 32)
                            words of this step's adjacency mask (bit k of word k / 32 = node k's rows / columns are zeroed, …_july.py:1627-1648), 32 bits per double   */
} gmpe_outputs;

int gmpe_abi_version(void);
const char* gmpe_last_error(void);

/* Observation width D, node feature count F and node count E for a config (no device needed). */
int gmpe_obs_dim(const gmpe_config* cfg);
int gmpe_node_feats(const gmpe_config* cfg);   /* 8; 7 for the rot_inv family and for graph_feat_type = 1 */
int gmpe_num_entities(const gmpe_config* cfg);
int gmpe_entity_table_width(const gmpe_config* cfg);   /* W of gmpe_outputs.entity_table: 2E + 4A (+ 2A rot_inv family) (+ 2 two_phase_graph) + ceil(E / 32) doubles per env */

/* Create the engine on HIP device `device`. Replaces N x `GraphMPEEnv(args)` + `env.seed(seed +
 * rank*1000)` (multiagent/MPE_env.py:56-84, onpolicy/scripts/train_mpe.py:21-43). */
int gmpe_create(const gmpe_config* cfg, int device, gmpe_handle** out);
int gmpe_destroy(gmpe_handle* h);

/* Parity mode: replay the reference's np.random draws. `tape_dev` is DEVICE memory, f64
 * [N, len_per_env] of [0,1) samples; draw k of env n is tape[n*len+k]. NULL returns to the
 * counter-based Philox4x32-10 stream keyed by (seed, env_id_base+n, k). */
int gmpe_set_rng_tape(gmpe_handle* h, const double* tape_dev, int64_t len_per_env);

/* Replaces GraphSubprocVecEnv.reset (env_wrappers.py:1006-1013 → environment.py:1066-1081 →
 * …_july.py:339-420). `env_mask_dev` (u8 [N], device) selects envs; NULL = all. */
int gmpe_reset(gmpe_handle* h, const uint8_t* env_mask_dev, const gmpe_outputs* out, void* stream);

/* Replaces GraphSubprocVecEnv.step (env_wrappers.py:991-1004 → graphworker :851-873 →
 * environment.py:1021-1063), including the worker's auto-reset: envs whose agents are all done
 * return their POST-reset obs/agent_id/node_obs/adj with the terminal reward/done.
 * `action_idx_dev`: i32 [N,A] discrete action index (argmax of the runner's one-hot,
 * environment.py:446). */
int gmpe_step(gmpe_handle* h, const int32_t* action_idx_dev, const gmpe_outputs* out, void* stream);

/* The same step for the envs [env_lo, env_hi) only; `action_idx_dev` and `out` are the WHOLE-batch arrays (rows outside the range are neither
 * read nor written). Envs are independent (one OS process each in the reference, env_wrappers.py:968-975), so ranges may be stepped on different
 * streams at different times — e.g. a runner that double-buffers two halves of the batch: while the policy works on one half's observations the
 * other half steps, and one half's latency chain runs under the other half's store drain. Not on the split big-E path (GMPE_ERR_UNSUPPORTED). */
int gmpe_step_envs(gmpe_handle* h, const int32_t* action_idx_dev, const gmpe_outputs* out, int32_t env_lo, int32_t env_hi, void* stream);
/* `num_steps` steps of `parts` (1..4) equal env ranges, each range on a side stream of its own (forked from / joined into `stream` once per call): the launch
 * shape of a runner that double-buffers ranges of the batch, with the open-loop action source of gmpe_step_many. Same results as gmpe_step_many. */
int gmpe_step_many_envs(gmpe_handle* h, const int32_t* actions_dev, int32_t num_steps, int32_t num_action_sets, const gmpe_outputs* out,
                        int32_t parts, void* stream);

/* `num_steps` consecutive steps enqueued by one call (no host round trip between steps; one launch, see gmpe_rollout_steps): step k uses
 * action set k % num_action_sets of `actions_dev` (i32 [num_action_sets, N, A]). Outputs are overwritten
 * by every step (same buffers), exactly as a host loop over gmpe_step would. Used for open-loop rollouts
 * (random-action benchmarking, scripted policies). */
int gmpe_step_many(gmpe_handle* h, const int32_t* actions_dev, int32_t num_steps, int32_t num_action_sets,
                   const gmpe_outputs* out, void* stream);
/* The same steps as ONE KERNEL LAUNCH PER STEP (the closed-loop launch shape, enqueued without host round trips; replays a graph
 * recorded by gmpe_step_many_prepare when there is one). gmpe_step_many falls back to this on the split big-E path, where the steps' chunk
 * pipelines are chained (gmpe_tuning.xstep): the side streams fork before the first step and join the caller's stream after the last one. */
int gmpe_step_many_launches(gmpe_handle* h, const int32_t* actions_dev, int32_t num_steps, int32_t num_action_sets,
                            const gmpe_outputs* out, void* stream);

/* Open-loop rollout in ONE launch (round 2): the K steps run inside a persistent kernel — each workgroup keeps the state of its
 * envs in LDS / registers from step to step (no reload, one write-back at the end) and the graph stores of step k drain under
 * step k+1's arithmetic. Results are bit-identical to K calls of gmpe_step (auto-resets included).
 * This is what the reference's collect loop does with a fixed action source: graph_mpe_runner.py:57-103 (`for step in
 * range(self.episode_length)`: envs.step -> GraphReplayBuffer.insert, onpolicy/utils/graph_buffer.py:168-251), minus the policy.
 * Output placement: step k writes slot (first_slot + k) % num_slots; slot s of an output lies `stride_*` ELEMENTS after slot 0
 * (the pointers in `slot0`). num_slots = 1 with zero strides = "every step overwrites the same buffers" (gmpe_step_many).
 * `masks` / `active_masks` (optional, f32 [slots][N,A], stride_masks apart) receive GraphReplayBuffer.insert's mask rules for the
 * step (see gmpe_masks_from_dones). Not available for handles on the split big-E path (gmpe_tuning.split): returns
 * GMPE_ERR_UNSUPPORTED there — use gmpe_step_many.
 * Performance note (round 3, profiles/r03_notes.md): with one slot every persistent workgroup rewrites its own output block each step; where a step's
 * outputs are far larger than the 256 MiB Infinity Cache that is markedly slower than slot-per-step storage (c4, 6 GB per step: 1122 us per step with one
 * slot, 929 with 4 slots, 868 with 26) — give big configurations the [T, ...] storage a rollout buffer has anyway. Outputs that fit the cache (c2 / c3:
 * 98 MB per step) are faster with one slot (absorbed by the cache) but are then not paid in DRAM writes. */
typedef struct gmpe_rollout {
    int32_t num_steps;          /* K >= 1                                                                  */
    int32_t num_action_sets;    /* S: step k uses action set k % S of actions_dev (i32 [S,N,A])            */
    int32_t num_slots;          /* >= 1                                                                    */
    int32_t first_slot;         /* in [0, num_slots)                                                       */
    int64_t stride_obs, stride_agent_id, stride_node_obs, stride_adj, stride_reward, stride_done, stride_info, stride_masks;
    float*  masks;              /* slot 0 of the masks, or NULL                                            */
    float*  active_masks;       /* slot 0 of the active_masks, or NULL                                     */
    int64_t stride_entity_table;/* ABI 3: elements (doubles) between consecutive slots of gmpe_outputs.entity_table */
} gmpe_rollout;
int gmpe_rollout_steps(gmpe_handle* h, const int32_t* actions_dev, const gmpe_rollout* plan, const gmpe_outputs* slot0, void* stream);

/* Optional: record the `num_steps` launches of gmpe_step_many(actions_dev, num_steps, num_action_sets, out) into a
 * hipGraph once (capture on a private stream + instantiate: milliseconds, not on the step path). Later
 * gmpe_step_many calls with the SAME pointers and counts replay it with one hipGraphLaunch on the caller's stream
 * (kernel-to-kernel dispatch overhead 3.6 -> 1.6 us at this launch shape, profiles/README.md); any other call takes
 * the plain launch loop. The action / output BUFFERS are baked in, their contents are read at replay time.
 * Since round 2 gmpe_step_many runs the rollout kernel above by default (gmpe_tuning.roll); a prepared graph is what it falls back to
 * when that is off (GMPE_ROLL=0) or unavailable (split path, per-launch timing). */
int gmpe_step_many_prepare(gmpe_handle* h, const int32_t* actions_dev, int32_t num_steps, int32_t num_action_sets,
                           const gmpe_outputs* out);

/* Same, taking the runner's float one-hot [N,A,n_actions] (graph_mpe_runner.py:375-377); the
 * argmax (np.argmax: first maximum) is fused into the step kernel. */
int gmpe_step_onehot(gmpe_handle* h, const float* onehot_dev, const gmpe_outputs* out, void* stream);

/* Safety-filter hook slot (multiagent/core.py:505-534, 692-736): in the reference `World.step` hands every agent's raw control
 * [omega, accel] (or [a_x, a_y]) to `safety_handle.apply_safety_filter` between `get_action()` and `update_agent_state` and
 * integrates the FILTERED control. The HJ / CBF filter itself is out of scope (value-function data and jax / cvxpy are absent); this
 * keeps its place in the step: when `ctrl_dev` (f64 [N,A,2], device, caller-owned) is set, agent (n,a) integrates ctrl_dev[n,a,:]
 * instead of its decoded action wherever `use_dev` (u8 [N,A]; NULL = everywhere) is non-zero — the `filtered` flag of the reference.
 * Units: the decoded control AFTER the x5 sensitivity (environment.py:460-463), i.e. what `agent.action.u` holds. An external
 * filter kernel reads the state through gmpe_field_device_ptr and runs on the same stream before gmpe_step. NULL removes the hook. */
int gmpe_set_control_override(gmpe_handle* h, const double* ctrl_dev, const uint8_t* use_dev);
/* Device pointer of a state field (layout in gmpe_field), valid for the life of the handle; for on-device consumers such as the
 * filter above. Reading it is ordered with the engine's launches only through the stream they share. */
int gmpe_field_device_ptr(gmpe_handle* h, int field, void** ptr_out);

/* Host <-> engine state copies (whole field, `bytes` must equal the field's size). */
int gmpe_field_bytes(const gmpe_handle* h, int field, size_t* bytes);
int gmpe_get_field(gmpe_handle* h, int field, void* host_dst, size_t bytes);
int gmpe_set_field(gmpe_handle* h, int field, const void* host_src, size_t bytes);

/* Learner-side edge set of onpolicy/algorithms/utils/gnn_new.py:329-358 (process_adj):
 * mask = (adj < max_edge_dist) & (adj > 0) on fp32, edges in (batch,row,col) lexicographic order,
 * node ids offset by batch*E. adj_dev: f32 [B,E,E]. Outputs: edge_index i32 [2,cap] (row 0 = src,
 * row 1 = dst), edge_attr f32 [cap], n_edges i32 [1] (device). If more than `cap` edges exist only
 * the first `cap` are written and n_edges still holds the true count. */
int gmpe_edges_from_adj(gmpe_handle* h, const float* adj_dev, int32_t batch, int32_t num_nodes,
                        float max_edge_dist, int32_t inclusive, int32_t* edge_index_dev,
                        float* edge_attr_dev, int32_t cap, int32_t* n_edges_dev, void* stream);

/* The same edge set computed from the COMPACT adjacency the engine writes with gmpe_outputs.adj_compact (adj_compact_dev: f32
 * [num_envs,E,E]): the `copies` (= A) per-agent graphs of an env are identical up to the id shift, so each matrix is read once and
 * the A copies of its edge list are emitted — output identical to gmpe_edges_from_adj on the materialised [num_envs*copies,E,E]
 * tensor, batch b = env*copies + copy. index64 != 0: edge_index is int64 [2,cap] (what torch.nonzero / PyG message passing use,
 * gnn_new.py:329-358), else int32. n_edges saturates at INT32_MAX. */
int gmpe_edges_from_adj_compact(gmpe_handle* h, const float* adj_compact_dev, int32_t num_envs, int32_t copies, int32_t num_nodes,
                                float max_edge_dist, int32_t inclusive, int32_t index64, void* edge_index_dev, float* edge_attr_dev,
                                int64_t cap, int32_t* n_edges_dev, void* stream);

/* Learner side of the compact rollout gather (replaces what GraphSubprocVecEnv.step_wait receives pickled from its workers, onpolicy/envs/env_wrappers.py:996-1004, for
 * the node features consumed by GraphReplayBuffer.insert, onpolicy/utils/graph_buffer.py:168-251): rebuild node_obs rows from entity tables
 * (gmpe_outputs.entity_table) with the engine's own arithmetic — same operations in the same order, -ffp-contract=off — so the result is BIT-IDENTICAL to the
 * node_obs the engine would have written (_get_entity_feat_relative …_july.py:1694-1771 / rot_inv.py:1690-1766, _get_entity_feat_global …_july.py:1672-1691,
 * including the ordered-visibility rule for re-drawn velocities). Needs no handle (the learner rank may own no envs): `cfg` supplies scenario, feature type and sizes.
 *   table_dev     f64 [num_blocks, envs_per_block, W]           (e.g. one rank's [T+1, N, W] rollout section)
 *   node_obs_dev  f32 [num_blocks, out_envs_per_block, A, E, F]  block t, env n -> out env out_env_offset + n (a rank's env range inside the global batch) */
int gmpe_expand_node_obs(const gmpe_config* cfg, int device, const double* table_dev, int64_t num_blocks, int64_t envs_per_block,
                         float* node_obs_dev, int64_t out_envs_per_block, int64_t out_env_offset, void* stream);
/* The same for the adjacency: the E x E matrix of every env-step from its entity table (positions + mask words) — f32(sqrt(dx^2 + dy^2)) with the engine's own
 * expression (World.calculate_distances, core.py:600-624), masked rows / columns zeroed (…_july.py:1627-1648) — bit-identical to gmpe_outputs.adj, so a rank need not
 * ship the matrix at all. adj_dev: f32 [num_blocks, out_envs_per_block, copies, E, E]; copies = 1: the compact form, copies = A: the materialised [.., A, E, E]. */
int gmpe_expand_adj(const gmpe_config* cfg, int device, const double* table_dev, int64_t num_blocks, int64_t envs_per_block,
                    float* adj_dev, int64_t out_envs_per_block, int64_t out_env_offset, int32_t copies, void* stream);

/* Rollout-buffer masks from a step's dones (GraphReplayBuffer.insert: onpolicy/utils/graph_buffer.py:223-251 with the runner's
 * rules graph_mpe_runner.py:85-90, 395-405): masks f32 [N,A] = 0 where done; active_masks f32 [N,A] = 0 where done unless all agents of
 * the env are done. Either output may be NULL. */
int gmpe_masks_from_dones(gmpe_handle* h, const uint8_t* done_dev, float* masks_dev, float* active_masks_dev, void* stream);

/* ---- Learner side of a rollout (handle-less, like gmpe_expand_node_obs): returns, advantages, stop-action rows ----
 * No allocation, no host synchronisation, every launch on `stream`: capturable in a hipGraph. Arrays are f32 device memory of
 * `lanes` = N*A values per slot (the reference's [.., N, A, 1]), consecutive slots `stride` elements apart.
 *
 * gmpe_compute_returns = GraphReplayBuffer.compute_returns (onpolicy/utils/graph_buffer.py:285-366), all four branches (flags), with
 * ValueNorm / PopArt denormalisation x * std + mean as two roundings (valuenorm.py:87-99, popart.py:101-111; device scalars, so the
 * caller's stream never waits on the host), and the head of GR_MAPPO.train (graph_mappo.py:294-304): raw advantages
 * returns[t] - denorm(value_preds[t]) and, optionally, (adv - mean) / (std + 1e-5) over the entries whose active_masks[t] != 0
 * (population std). Returns and raw advantages are bit-identical to the reference's float32 NumPy (its operation order, no contraction,
 * f32(gamma * gae_lambda) rounded from the double product); mean / std are accumulated in double from per-wave partials merged in a
 * fixed order (bitwise reproducible; NaN when no entry is active, like np.nanmean). Side effects as the reference: with GAE
 * value_preds[T] = next_value, without it returns[T] = next_value. One launch, three with `normalized`. */
#define GMPE_RETURNS_GAE 1                  /* args.use_gae                                                                    */
#define GMPE_RETURNS_PROPER_TIME_LIMITS 2   /* args.use_proper_time_limits: bad_masks                                          */
#define GMPE_RETURNS_ADVANTAGES_ONLY 4      /* skip the recurrence: advantages from the returns / value_preds as they are (train) */
typedef struct gmpe_returns_plan {
    int32_t num_steps;          /* T >= 1                                                                                       */
    int32_t flags;              /* GMPE_RETURNS_*                                                                               */
    int64_t lanes;              /* N*A >= 1                                                                                     */
    int64_t stride;             /* elements between consecutive slots of every array below (>= lanes)                          */
    double gamma, gae_lambda;
    const float* rewards;       /* [T]    (not read with ADVANTAGES_ONLY)                                                       */
    const float* masks;         /* [T+1]  (idem)                                                                                */
    const float* bad_masks;     /* [T+1]  PROPER_TIME_LIMITS only                                                               */
    float* value_preds;         /* [T+1]  GAE: slot T receives next_value                                                       */
    float* returns;             /* [T+1]  written for slots 0..T-1; without GAE slot T receives next_value                      */
    const float* next_value;    /* [lanes] (not read with ADVANTAGES_ONLY)                                                      */
    const float* denorm_mean;   /* f32 [1] device: the normaliser's mean, or NULL (no denormalisation)                          */
    const float* denorm_std;    /* f32 [1] device: sqrt(var); set exactly when denorm_mean is                                   */
    float* advantages;          /* [T] raw advantages, or NULL                                                                  */
    const float* active_masks;  /* [T+1] (slots 0..T-1 read): needed with `normalized`                                          */
    float* normalized;          /* [T] normalised advantages, or NULL; may be `advantages` itself (in place)                    */
    void* workspace;            /* device scratch of gmpe_returns_workspace_bytes(lanes) bytes: needed with `normalized`        */
    size_t workspace_bytes;
} gmpe_returns_plan;
int gmpe_returns_workspace_bytes(int64_t lanes, size_t* bytes_out);
int gmpe_compute_returns(int device, const gmpe_returns_plan* plan, void* stream);

/* The same call for a learner whose batch lies in `world` shards (data-parallel ranks, or pieces of a batch inside one process): the advantage
 * statistics are those of the WHOLE batch, the same bits on every shard. Two phases around one exchange the caller makes (an all-gather of `local`):
 *   GMPE_SHARD_LOCAL  everything gmpe_compute_returns does up to the statistics (recurrence or advantages-only; returns, side effects, raw advantages),
 *                     the per-wave Welford partials merged in gmpe_compute_returns' fixed order, written to `local` as (n, mean, M2). Nothing is
 *                     normalised: the raw advantages stay in `advantages` (in `normalized` when `advantages` is NULL) until APPLY.
 *   GMPE_SHARD_APPLY  the `world` triples of `all` merged with the same Chan merge as a left fold in index order (an empty side is skipped, so a shard
 *                     with no active entry, n = 0, changes nothing), turned into (mean, std + 1e-5) by gmpe_compute_returns' own code, and this
 *                     shard's raw advantages normalised with them. Run it once per LOCAL: in place it would normalise twice.
 * `base.normalized`, `base.active_masks` and `base.workspace` are required in both phases, and both take the same `base`. Neither phase allocates, uses
 * atomics or waits for the device; both are capturable. With world = 1 and all == local, LOCAL then APPLY gives gmpe_compute_returns' outputs bit for bit. */
#define GMPE_SHARD_LOCAL 0
#define GMPE_SHARD_APPLY 1
#define GMPE_SHARD_MAX_WORLD 4096
#define GMPE_RETURNS_SHARD_STATS 3          /* doubles per shard: n, mean, M2                                                   */
typedef struct gmpe_returns_shard_plan {
    gmpe_returns_plan base;     /* as for gmpe_compute_returns, with normalized, active_masks and workspace set                 */
    int32_t phase;              /* GMPE_SHARD_LOCAL or GMPE_SHARD_APPLY                                                         */
    int32_t world;              /* shards, 1 .. GMPE_SHARD_MAX_WORLD                                                            */
    double* local;              /* f64 [3] device, 8-byte aligned: written by LOCAL (not read by APPLY)                         */
    const double* all;          /* f64 [world, 3] device, 8-byte aligned: read by APPLY in index order (not read by LOCAL)      */
} gmpe_returns_shard_plan;
int gmpe_compute_returns_shard(int device, const gmpe_returns_shard_plan* plan, void* stream);

/* available_actions of the shipped training loop (GMPERunner.run + collect_with_mask, graph_mpe_runner.py:73-141, 263-335, stored by
 * GraphReplayBuffer.insert at slot step + 1, graph_buffer.py:249-250): the availability the policy acts with at step t >= 1 is a function of
 * the dones of step t - 1 — a one-hot "stop" row at n_actions / 2 for an agent that was done, a row of ones otherwise (every agent of an env
 * whose agents were all done gets the stop row, although that env has auto-reset) — and at step 0 it is all ones.
 * Positions are the steps of one episode, t = (first + k) % num_positions for k < count: position t reads dones slot t - 1
 * (u8 [lanes], `stride_dones` elements apart from slot 0) and writes f32 [lanes, n_actions] at available_actions + t * stride_out. */
typedef struct gmpe_avail_plan {
    const uint8_t* dones;       /* slot 0 of the dones (position t reads slot t - 1)                                           */
    float* available_actions;   /* the rows of position 0 (the buffer's slot 1)                                                */
    int64_t lanes;              /* N*A                                                                                         */
    int32_t n_actions;
    int32_t num_positions;      /* T (episode length)                                                                          */
    int32_t first;              /* position of the first step, in [0, T)                                                       */
    int32_t count;              /* steps (>= 0; more than T write every position once)                                         */
    int64_t stride_dones, stride_out;
} gmpe_avail_plan;
int gmpe_available_actions_from_dones(int device, const gmpe_avail_plan* plan, void* stream);

/* The learner's fields of one rollout step (GMPERunner.insert + GraphReplayBuffer.insert, graph_mpe_runner.py:384-392, graph_buffer.py:229-234) in one launch:
 *   value_preds[t] = values;  actions[t] = float32(actions_in);  action_log_probs[t] = log_probs_in;
 *   rnn_states[t + 1] = rnn_in, rnn_states_critic[t + 1] = rnn_critic_in, with the rows of every lane done at step t (dones[t][lane] != 0) zeroed.
 * The zeroing is per agent (the runner's `rnn_states[dones] = 0`, not dones_env). An input left NULL skips its field; a field's output is required
 * when its input is given. Slot s of an array is at its slot-0 pointer + s * stride elements; a slot's rows are contiguous ([lanes, k] / [lanes, R, H]).
 * Inputs are the policy's outputs, contiguous: values f32 [lanes], actions_in int64 or f32 [lanes, k], log_probs_in f32 [lanes, k], rnn_in f32 [lanes, R, H],
 * rnn_critic_in f32 [lanes, R, hidden_critic]. dones is read from the device (written by the step before on the same stream): no host synchronisation.
 * Every argument the host can see is checked before any device call; one launch on `stream` (none when no input is given). */
typedef struct gmpe_learner_plan {
    int64_t lanes;              /* N*A >= 1                                                                                      */
    int32_t t;                  /* step, 0 <= t < num_steps                                                                      */
    int32_t num_steps;          /* T (episode length): value_preds / rnn arrays hold T + 1 slots, actions / log-probs T          */
    int32_t recurrent_n;        /* R, 1 .. 64                                                                                    */
    int32_t hidden;             /* H of rnn_states, 1 .. 65536                                                                   */
    int32_t hidden_critic;      /* H of rnn_states_critic, 1 .. 65536                                                            */
    int32_t act_dim;            /* k of actions / action_log_probs, 1 .. 64                                                      */
    int32_t actions_int64;      /* 1: actions_in is int64 (what the policy returns), 0: float32                                  */
    int32_t reserved;           /* 0                                                                                             */
    const uint8_t* dones;       /* slot 0 of u8 [T][lanes]; needed with rnn_in or rnn_critic_in                                  */
    const float* values;        /* [lanes] or NULL                                                                               */
    const void* actions_in;     /* [lanes, k] or NULL (8-byte aligned when int64)                                               */
    const float* log_probs_in;  /* [lanes, k] or NULL                                                                            */
    const float* rnn_in;        /* [lanes, R, H] or NULL                                                                         */
    const float* rnn_critic_in; /* [lanes, R, hidden_critic] or NULL                                                             */
    float* value_preds;         /* slot 0 of [T+1][lanes]                                                                        */
    float* actions;             /* slot 0 of [T][lanes, k]                                                                       */
    float* action_log_probs;    /* slot 0 of [T][lanes, k]                                                                       */
    float* rnn_states;          /* slot 0 of [T+1][lanes, R, H]                                                                  */
    float* rnn_states_critic;   /* slot 0 of [T+1][lanes, R, hidden_critic]                                                      */
    int64_t stride_dones, stride_value_preds, stride_actions, stride_action_log_probs, stride_rnn_states, stride_rnn_states_critic;
                                /* elements between consecutive slots, at least one slot each (slots do not overlap)             */
} gmpe_learner_plan;
int gmpe_insert_learner(int device, const gmpe_learner_plan* plan, void* stream);

/* Everything that follows the env step of rollout step t = learner.t and is a function of dones[t - 1], dones[t] and the policy's outputs alone (the
 * "after the step" half of GMPERunner.insert, graph_mpe_runner.py:384-405, with collect_with_mask's stop rows), in ONE launch on `stream`:
 *   the learner's fields, exactly as gmpe_insert_learner writes them for `learner` (its inputs are all optional here too);
 *   masks[t + 1][q] = dones[t][q] ? 0 : 1;  active_masks[t + 1][q] = 0 where lane q is done and not every agent of its env is, else 1
 *     (gmpe_masks_from_dones' rule; lane q belongs to env q / num_agents);
 *   position t of available_actions (the buffer's slot t + 1), exactly as gmpe_available_actions_from_dones writes it with first = t, count = 1:
 *     all ones at t = 0, else the one-hot row at n_actions / 2 for a lane with dones[t - 1] != 0 and ones for every other lane;
 *   *draw_dev += draw_inc by one thread (gmpe_act_sample's counter: the step's sampling launch, given draw_inc = 0, has read it earlier on the stream).
 * Any dones byte != 0 counts as done. An output left NULL is skipped. Plain stores, no atomics, no allocation, no host synchronisation: capturable.
 * Every argument the host can see is checked before any device call; always exactly one launch, also when no learner input is given. */
typedef struct gmpe_step_tail_plan {
    gmpe_learner_plan learner;      /* as for gmpe_insert_learner; here `dones` is required (the masks read it)                      */
    int32_t num_agents;             /* A >= 1; lanes % A == 0; an env's lanes are consecutive                                        */
    int32_t n_actions;              /* with available_actions: 1 .. 64, stop row at n_actions / 2                                    */
    float* masks;                   /* slot 0 of f32 [T+1][lanes], or NULL                                                           */
    float* active_masks;            /* slot 0 of f32 [T+1][lanes], or NULL                                                           */
    float* available_actions;       /* rows of position 0 (the buffer's slot 1), as gmpe_avail_plan's, or NULL                       */
    int64_t stride_masks, stride_active_masks, stride_available_actions;   /* elements between slots, each at least one slot        */
    uint64_t* draw_dev;             /* u64 [1], 8-byte aligned, or NULL                                                              */
    uint64_t draw_inc;              /* added to *draw_dev                                                                            */
} gmpe_step_tail_plan;
int gmpe_step_tail(int device, const gmpe_step_tail_plan* plan, void* stream);

/* The loss arithmetic of one PPO minibatch (GR_MAPPO.ppo_update, onpolicy/algorithms/graph_mappo.py:176-207 + cal_value_loss :89-117) between the policy
 * head's logits / the critic's values and the two scalars the reference calls .backward() on, with their gradients, in four launches on `stream`
 * (no atomics, no allocation, no host synchronisation; capturable):
 *   the masked categorical of Categorical.forward + ACTLayer.evaluate_actions (distributions.py:84-91, act.py:212-220): logits at finfo(float32).min where
 *   available_actions == 0, log-prob of the action, entropy; ratio = exp(logp - old_action_log_probs), the clipped surrogate; the value loss (huber as
 *   util.py:24-27 writes it, one-sided: zero for errors below -delta; or mse), clipped or not, with ValueNorm.update applied to the three state scalars
 *   BEFORE returns are normalised (valuenorm.py:56-85). Means are over active_masks (sum(x * m) / sum(m)) or plain, per flag; a zero mask sum gives NaN.
 * Per-row arithmetic is float32 as the reference computes it; sums over rows are double, merged in a fixed order: the same rows give the same bits
 * wherever they lie in memory. Every [rows, 1] array is a contiguous f32 [rows]; logits / available_actions / grad_logits are contiguous [rows, n_actions]
 * (read and written in 16-byte units when all three are 16-byte aligned, in 4-byte units otherwise). */
#define GMPE_PPO_POLICY_ACTIVE_MASKS 1   /* args.use_policy_active_masks: policy loss and entropy are means over active_masks        */
#define GMPE_PPO_VALUE_ACTIVE_MASKS 2    /* args.use_value_active_masks                                                               */
#define GMPE_PPO_CLIPPED_VALUE_LOSS 4    /* args.use_clipped_value_loss: max(original, clipped)                                       */
#define GMPE_PPO_HUBER_LOSS 8            /* args.use_huber_loss (else mse)                                                            */
#define GMPE_PPO_VALUENORM 16            /* args.use_valuenorm: update the three scalars, then normalise returns with them            */
#define GMPE_PPO_MAX_ACTIONS 64          /* n_actions above this: GMPE_ERR_INVALID_ARG                                                */
#define GMPE_PPO_OUT_POLICY_LOSS 0       /* columns of `out` (f64)                                                                    */
#define GMPE_PPO_OUT_DIST_ENTROPY 1
#define GMPE_PPO_OUT_ACTOR_LOSS 2        /* policy_loss - entropy_coef * dist_entropy                                                 */
#define GMPE_PPO_OUT_VALUE_LOSS 3
#define GMPE_PPO_OUT_RATIO_MEAN 4        /* imp_weights.mean()                                                                        */
#define GMPE_PPO_OUT_DENOM_POLICY 5      /* sum(active_masks) or rows                                                                 */
#define GMPE_PPO_OUT_DENOM_VALUE 6
#define GMPE_PPO_NUM_OUT 7
typedef struct gmpe_ppo_loss_plan {
    int64_t rows;                       /* B >= 1                                                                                     */
    int32_t n_actions;                  /* K, 1 .. GMPE_PPO_MAX_ACTIONS                                                               */
    int32_t flags;                      /* GMPE_PPO_*                                                                                 */
    int32_t actions_int64;              /* 1: actions is int64 [rows], 0: f32 [rows] (truncated like .long())                         */
    int32_t reserved;                   /* 0                                                                                          */
    double clip_param, huber_delta, entropy_coef;
    double beta, epsilon;               /* ValueNorm's (0.99999, 1e-5); read with GMPE_PPO_VALUENORM                                  */
    const float* logits;                /* [rows, K] the head's linear output, before masking                                         */
    const float* values;                /* [rows]                                                                                     */
    const void* actions;                /* [rows]; values outside 0 .. K-1 are the caller's error (read as the nearest column)        */
    const float* available_actions;     /* [rows, K] or NULL (all available)                                                          */
    const float* old_action_log_probs;  /* [rows]                                                                                     */
    const float* adv_targ;              /* [rows]                                                                                     */
    const float* value_preds;           /* [rows]                                                                                     */
    const float* returns;               /* [rows]                                                                                     */
    const float* active_masks;          /* [rows]                                                                                     */
    float* running_mean;                /* f32 [1] each, updated in place; all three set exactly with GMPE_PPO_VALUENORM              */
    float* running_mean_sq;
    float* debiasing_term;
    double* out;                        /* f64 [GMPE_PPO_NUM_OUT]                                                                     */
    float* grad_logits;                 /* [rows, K] d actor_loss / d logits (already divided by the denominator)                     */
    float* grad_values;                 /* [rows]    d value_loss / d values                                                          */
    float* action_log_probs;            /* [rows] or NULL                                                                             */
    float* imp_weights;                 /* [rows] or NULL                                                                             */
    void* workspace;                    /* device scratch of gmpe_ppo_loss_workspace_bytes(rows) bytes, 8-byte aligned                */
    size_t workspace_bytes;
} gmpe_ppo_loss_plan;
int gmpe_ppo_loss_workspace_bytes(int64_t rows, size_t* bytes_out);
int gmpe_ppo_loss(int device, const gmpe_ppo_loss_plan* plan, void* stream);

/* The same minibatch lying in `world` shards (see gmpe_compute_returns_shard): the means are over the WHOLE minibatch and ValueNorm.update sees its
 * returns, the same bits on every shard.
 *   GMPE_SHARD_LOCAL  the double sums of returns, returns^2 and active_masks over this shard's rows, merged in gmpe_ppo_loss' fixed order, and the
 *                     row count, written to `local` as four doubles. The ValueNorm scalars are not touched.
 *   GMPE_SHARD_APPLY  the rows of `all` added sequentially in index order in double; the denominators, the ValueNorm update and the normalisation
 *                     scalars from those GLOBAL sums and the global row count by gmpe_ppo_loss' own code; then gmpe_ppo_loss' row pass over this
 *                     shard's rows. `out` holds this shard's sums divided by the global denominators (ratio_mean: by the global row count), so
 *                     the rows of all shards ADD UP to the scalars of the whole minibatch; the two DENOM columns hold the global denominators;
 *                     grad_logits / grad_values are rows of the gradient of the global loss; every replica's ValueNorm receives the same update.
 * Both phases take the same `base`; neither allocates, uses atomics or waits for the device; both are capturable. With world = 1 and all == local,
 * LOCAL then APPLY gives gmpe_ppo_loss' outputs and ValueNorm state bit for bit. gmpe_ppo_loss_popart has no sharded form. */
#define GMPE_PPO_SHARD_STATS 4           /* doubles per shard: sum returns, sum returns^2, sum active_masks, rows                     */
typedef struct gmpe_ppo_loss_shard_plan {
    gmpe_ppo_loss_plan base;            /* as for gmpe_ppo_loss                                                                       */
    int32_t phase;                      /* GMPE_SHARD_LOCAL or GMPE_SHARD_APPLY                                                       */
    int32_t world;                      /* shards, 1 .. GMPE_SHARD_MAX_WORLD                                                          */
    double* local;                      /* f64 [4] device, 8-byte aligned: written by LOCAL (not read by APPLY)                       */
    const double* all;                  /* f64 [world, 4] device, 8-byte aligned: read by APPLY in index order (not read by LOCAL)    */
} gmpe_ppo_loss_shard_plan;
int gmpe_ppo_loss_shard(int device, const gmpe_ppo_loss_shard_plan* plan, void* stream);

/* The same minibatch with --use_popart: the value normaliser is the critic's output layer v_out = PopArt(hidden, 1)
 * (onpolicy/algorithms/utils/popart.py, graph_mappo.py:63-64), so the line to the critic is its FEATURES [rows, hidden], not its values. In four
 * launches on `stream` (no atomics, no allocation, no host synchronisation; capturable), in the reference's order:
 *   1. values = critic_features . weight + bias with the weights as they are BEFORE the update (evaluate_actions runs first, graph_mappo.py:160-172);
 *   2. PopArt.update(returns) (popart.py:62-83) in float32 over ALL rows: mean, mean_sq, debiasing_term move in place;
 *      stddev' = clamp(sqrt(mean_sq - mean^2), 1e-4) from the RAW statistics (NaN stays NaN); weight' = (weight * stddev) / stddev';
 *      bias' = ((stddev * bias + mean') - mean') / stddev' — old_mean is an alias of the updated mean there, and that is restated, not corrected;
 *   3. the losses of gmpe_ppo_loss with returns normalised by the DEBIASED statistics (popart.py:85-99: mean / clamp(debiasing_term, epsilon),
 *      sqrt(clamp(mean_sq / ... - mean_d^2, 1e-2)));
 *   4. d value_loss / d critic_features, d weight, d bias, all through the pre-update weights;
 *   5. weight', bias', stddev' are published by the last launch: each *_out may be the very pointer of its input (rescaled in place), and is written
 *      only after every row has read the input. Any other overlap between arrays is the caller's error.
 * The dot product of a row is float32 in one fixed order that depends on `hidden` alone: columns in quads (4q .. 4q+3), quad q on lane q mod L of L
 * lanes (L = the power of two >= ceil(hidden / 4), at most 64), a lane adds its products in column order, the L lanes are added as a tree (lower lane
 * the left operand), then the bias. critic_features and grad_features move in 16-byte units when hidden % 4 == 0 and both are 16-byte aligned, in
 * 4-byte units otherwise; the bits do not depend on which. grad_weight / grad_bias are double sums over rows, rounded to float32 once. */
#define GMPE_POPART_MAX_HIDDEN 1024
typedef struct gmpe_popart_loss_plan {
    int64_t rows;                       /* B >= 1                                                                                     */
    int32_t n_actions;                  /* K, 1 .. GMPE_PPO_MAX_ACTIONS                                                               */
    int32_t hidden;                     /* H, 1 .. GMPE_POPART_MAX_HIDDEN                                                             */
    int32_t flags;                      /* the four boolean GMPE_PPO_* flags; GMPE_PPO_VALUENORM is not accepted                      */
    int32_t actions_int64;              /* as gmpe_ppo_loss_plan                                                                      */
    double clip_param, huber_delta, entropy_coef;
    double beta, epsilon;               /* PopArt's (0.99999, 1e-5)                                                                   */
    const float* logits;                /* [rows, K]                                                                                  */
    const float* critic_features;       /* [rows, H] the input of v_out                                                               */
    const void* actions;                /* [rows]                                                                                     */
    const float* available_actions;     /* [rows, K] or NULL                                                                          */
    const float* old_action_log_probs;  /* [rows]                                                                                     */
    const float* adv_targ;              /* [rows]                                                                                     */
    const float* value_preds;           /* [rows]                                                                                     */
    const float* returns;               /* [rows]                                                                                     */
    const float* active_masks;          /* [rows]                                                                                     */
    const float* weight;                /* [H]  v_out.weight, read                                                                    */
    const float* bias;                  /* [1]  v_out.bias, read                                                                      */
    const float* stddev;                /* [1]  v_out.stddev, read                                                                    */
    float* mean;                        /* f32 [1] each, updated in place                                                             */
    float* mean_sq;
    float* debiasing_term;
    float* weight_out;                  /* [H], [1], [1]: the rescaled layer; each may be the pointer of its input                    */
    float* bias_out;
    float* stddev_out;
    float* values_out;                  /* [rows] or NULL: what v_out gave with the pre-update weights                                */
    double* out;                        /* f64 [GMPE_PPO_NUM_OUT]                                                                     */
    float* grad_logits;                 /* [rows, K] d actor_loss / d logits                                                          */
    float* grad_features;               /* [rows, H] d value_loss / d critic_features                                                 */
    float* grad_weight;                 /* [H]       d value_loss / d weight                                                          */
    float* grad_bias;                   /* [1]       d value_loss / d bias                                                            */
    float* action_log_probs;            /* [rows] or NULL                                                                             */
    float* imp_weights;                 /* [rows] or NULL                                                                             */
    void* workspace;                    /* device scratch of gmpe_ppo_loss_popart_workspace_bytes(rows, hidden) bytes, 8-byte aligned */
    size_t workspace_bytes;
} gmpe_popart_loss_plan;
int gmpe_ppo_loss_popart_workspace_bytes(int64_t rows, int32_t hidden, size_t* bytes_out);
int gmpe_ppo_loss_popart(int device, const gmpe_popart_loss_plan* plan, void* stream);

/* The rollout half of the same action head: ACTLayer.forward (onpolicy/algorithms/utils/act.py:107-113) — the masked Categorical
 * (distributions.py:84-91), sample() or mode() (:15-16, 27-28), log_probs (:18-25) — and what the runner makes of the action for the env and the buffer
 * (graph_mpe_runner.py:299-320, 356-377), in ONE launch on `stream` over rows = N*A rows of n_actions <= GMPE_PPO_MAX_ACTIONS float32 logits (no
 * allocation, no host synchronisation; capturable).
 *   Availability of a row, from at most one source: available_actions (f32 [rows, K], non-zero = available); or dones_prev (u8 [rows]) with stop_action —
 *   a row whose dones_prev is non-zero may only take stop_action, every other row everything: collect_with_mask's rule (graph_mpe_runner.py:270-286), what
 *   gmpe_available_actions_from_dones writes, without any [rows, K] array; or neither (everything available). A row with no available action is the
 *   reference's uniform row over all K actions (every log-prob 0, as gmpe_ppo_loss computes it) and is sampled over all K.
 *   Distribution: the float32 arithmetic of gmpe_ppo_loss's policy row in its order; log_probs[r] is bit-identical to the action_log_probs gmpe_ppo_loss
 *   returns for the same logits, availability and action.
 *   Sampling (deterministic == 0): u = philox(seed, env_id_base + r / num_agents, 2^63 | (draw * num_agents + r % num_agents)), the env streams' generator
 *   (gmpe_create) with the top counter bit set, so the actions do not depend on how envs are spread over calls, handles or devices; the action is the
 *   first available j whose running float32 sum of probabilities c_j has (double)c_j > u, else the mode. An unavailable action is never returned.
 *   deterministic == 1 (FixedCategorical.mode): the first index of the largest masked logit.
 *   Counter: with draw_dev (u64 [1] on the device) the rows use *draw_dev + draw and a second one-thread launch then adds draw_inc to *draw_dev, so a
 *   captured graph draws fresh numbers at every replay; without it, or with draw_inc == 0 (the caller advances the counter itself: gmpe_step_tail), there
 *   is exactly one launch.
 * logits / available_actions are contiguous [rows, K], read in 16-byte units when both are 16-byte aligned, in 4-byte units otherwise. Every argument
 * the host can see is checked before any device call. */
typedef struct gmpe_act_plan {
    int64_t rows;                       /* N*A >= 1                                                                                   */
    int32_t n_actions;                  /* K, 1 .. GMPE_PPO_MAX_ACTIONS                                                               */
    int32_t num_agents;                 /* A >= 1: row r is agent r % A of env env_id_base + r / A                                    */
    int32_t stop_action;                /* 0 .. K-1; read with dones_prev                                                             */
    int32_t deterministic;              /* 1: the mode, 0: a sample                                                                   */
    int32_t env_id_base;                /* global id of the env of row 0 (gmpe_config.env_id_base of the handle that steps these rows) */
    int32_t reserved;                   /* 0                                                                                          */
    uint64_t seed;                      /* gmpe_config.seed                                                                           */
    uint64_t draw;                      /* call counter: one value per act of the rollout                                             */
    uint64_t draw_inc;                  /* added to *draw_dev after the rows have read it                                             */
    uint64_t* draw_dev;                 /* u64 [1] on the device, 8-byte aligned, or NULL                                             */
    const float* logits;                /* [rows, K] the head's linear output, before masking                                         */
    const float* available_actions;     /* [rows, K] or NULL                                                                          */
    const uint8_t* dones_prev;          /* [rows] or NULL; not together with available_actions                                        */
    int32_t* action_idx;                /* [rows] what gmpe_step takes                                                                */
    float* log_probs;                   /* [rows]; may point into the buffer's action_log_probs[t]                                    */
    float* actions_f32;                 /* [rows] or NULL; may point into the buffer's actions[t]                                     */
    int64_t* actions_i64;               /* [rows] or NULL (what the policy returns), 8-byte aligned                                   */
} gmpe_act_plan;
int gmpe_act_sample(int device, const gmpe_act_plan* plan, void* stream);

/* ---- The policy's action head (handle-less): the Linear in front of the masked categorical above ----
 * Categorical.linear of a single Discrete ACTLayer (onpolicy/algorithms/utils/act.py:27-29, distributions.py:72-91): logits = features W^T + b with
 * weight [K, hidden], bias [K], float32, contiguous, hidden == 64 and 1 <= K <= GMPE_PPO_MAX_ACTIONS; everything else is GMPE_ERR_INVALID_ARG with the
 * function and the field in gmpe_last_error, before any launch. No allocation, no atomics, no host synchronisation; every launch on `stream`; capturable.
 *
 * gmpe_head_forward, ONE launch:
 *   logits_out[r, k] = the fmaf chain that starts at bias[k] and runs over h = 0 .. 63 ascending of features[r, h] * weight[k, h].
 *   A row's bits are a function of that row and the parameters alone: not of rows, not of the row's place in the call, not of the width of the loads
 *   (16-byte units where an array is 16-byte aligned, 4-byte units otherwise).
 * gmpe_head_backward, at most THREE launches, from grad_logits [rows, K] (features and weight as in forward; bias and logits_out are not read):
 *   grad_features[r, h] = the fmaf chain from 0.0f over k = 0 .. K-1 ascending of grad_logits[r, k] * weight[k, h]: a function of the row alone;
 *   grad_weight[k, h]   = sum over r of grad_logits[r, k] * features[r, h]: the rows are cut into P = min(128, ceil(rows / 32)) contiguous parts of
 *                         ceil(rows / P) rows; a part's exact double products are added in ascending row order, the parts in ascending part order, and
 *                         the sum is rounded to float32 once;
 *   grad_bias[k]        = sum over r of grad_logits[r, k] in double: within a tile of 256 rows four runs of 64 rows, each ascending, added in run order;
 *                         the tiles as 16 interleaved slices (slice s: tiles s, s + 16, ... ascending), the slices in slice order; rounded once.
 *   So the order is a function of rows alone and two calls give the same bits. Each of the three outputs may be NULL and is then not formed.
 * Workspace (backward only; gmpe_head_workspace_bytes is the single source of its size; its contents before the call do not matter), in this order:
 *   f64 [P][64][64] the parts' blocks, f64 [ceil(rows / 256)][64] the tiles' column sums. A forward-only plan needs none.
 *
 * gmpe_act_head, the rollout form: gmpe_act_sample with act_plan->logits == NULL (anything else is refused) and the logits formed in the launch from
 * head_plan->features, weight and bias (rows and n_actions of the two plans must agree; the head plan's gradient fields and workspace are not read).
 * Exactly ONE launch, plus gmpe_act_sample's one-thread counter launch when draw_dev is given and draw_inc != 0. The logits are the dot product of gmpe_head_forward (one
 * device function) and the row's routine is gmpe_act_sample's (one device function): action_idx, log_probs, actions_f32, actions_i64 — and logits_out,
 * written when it is not NULL — are bit for bit what gmpe_head_forward followed by gmpe_act_sample gives. With gmpe_ppo_loss recomputing log_probs from
 * gmpe_head_forward's logits, an unchanged policy has importance weights of exactly 1 whatever the two batch shapes. */
typedef struct gmpe_head_plan {
    int64_t rows;                       /* >= 1                                                                                       */
    int32_t n_actions;                  /* K, 1 .. GMPE_PPO_MAX_ACTIONS                                                               */
    int32_t hidden;                     /* 64                                                                                         */
    const float* features;              /* [rows, 64] the actor features                                                              */
    const float* weight;                /* [K, 64]                                                                                    */
    const float* bias;                  /* [K]; forward and gmpe_act_head                                                             */
    float* logits_out;                  /* [rows, K]; forward: required; gmpe_act_head: or NULL; backward: not read                   */
    const float* grad_logits;           /* [rows, K]; backward only                                                                   */
    float* grad_features;               /* [rows, 64] or NULL; backward only                                                          */
    float* grad_weight;                 /* [K, 64] or NULL; backward only                                                             */
    float* grad_bias;                   /* [K] or NULL; backward only                                                                 */
    void* workspace;                    /* gmpe_head_workspace_bytes(rows, K, 1) bytes, 8-byte aligned; backward only                 */
    size_t workspace_bytes;
} gmpe_head_plan;
/* want_backward == 0: 0 bytes. The size depends on rows alone; n_actions is checked. */
int gmpe_head_workspace_bytes(int64_t rows, int32_t n_actions, int32_t want_backward, size_t* bytes_out);
int gmpe_head_forward(int device, const gmpe_head_plan* plan, void* stream);
int gmpe_head_backward(int device, const gmpe_head_plan* plan, void* stream);
int gmpe_act_head(int device, const gmpe_act_plan* act_plan, const gmpe_head_plan* head_plan, void* stream);

/* ---- The critic's value head (handle-less): v_out of GR_Critic, an nn.Linear(64, 1) or a PopArt(64, 1) read as one ----
 * values = features W^T + b (onpolicy/algorithms/graph_actor_critic.py:395) with weight [1, hidden], bias [1], float32, contiguous, hidden == 64;
 * everything else is GMPE_ERR_INVALID_ARG with the function and the field in gmpe_last_error, before any launch. No allocation, no atomics, no host
 * synchronisation; every launch on `stream`; capturable.
 *
 * gmpe_value_forward, ONE launch:
 *   values_out[r] = the dot product gmpe_ppo_loss_popart evaluates at hidden == 64, bit for bit: a row is held by 16 lanes, lane c holding columns
 *   4c .. 4c+3; acc = 0.0f, then acc = acc + features[r, 4c + i] * weight[4c + i] for i = 0 .. 3, multiply and add each rounded on its own; the 16 lanes
 *   by an xor tree over offsets 1, 2, 4, 8 with the lower lane as the left operand; then + bias. A row's bits are a function of that row and the
 *   parameters alone: not of rows, not of the row's place in the call, not of the width of the loads (16-byte units where features is 16-byte aligned,
 *   4-byte units otherwise). So the value_preds a rollout stores are what gmpe_ppo_loss_popart recomputes on a minibatch of any other size.
 * gmpe_value_backward, at most TWO launches, from grad_values [rows] (features and weight as in forward; bias and values_out are not read):
 *   grad_features[r, j] = grad_values[r] * weight[j], one float32 product;
 *   grad_weight[j]      = sum over r of grad_values[r] * features[r, j], grad_bias = sum over r of grad_values[r], of exact double products: within a
 *                         tile of 256 rows, wave w (rows 64w .. 64w+63) adds the rows 4p + s of each s = 0 .. 3 over p = 0 .. 15 ascending, the four s by
 *                         an xor tree (s ^ 1, then s ^ 2; the lower the left operand), the four waves in wave order; the tiles as 16 interleaved slices
 *                         (slice q: tiles q, q + 16, ... ascending), the slices in slice order; rounded to float32 once.
 *   So the order is a function of rows alone and two calls give the same bits. Each of the three outputs may be NULL and is then not formed.
 * Workspace (backward only; gmpe_value_workspace_bytes is the single source of its size; its contents before the call do not matter):
 *   f64 [ceil(rows / 256)][80] the tiles' column sums (64 weight columns, the bias column, padding). A forward-only plan needs none. */
typedef struct gmpe_value_plan {
    int64_t rows;                       /* >= 1                                                                                       */
    int32_t hidden;                     /* 64                                                                                         */
    int32_t reserved;
    const float* features;              /* [rows, 64] the critic features                                                             */
    const float* weight;                /* [1, 64]                                                                                    */
    const float* bias;                  /* [1]; forward only                                                                          */
    float* values_out;                  /* [rows]; forward: required, may point into the buffer's value_preds[t]; backward: not read  */
    const float* grad_values;           /* [rows]; backward only                                                                      */
    float* grad_features;               /* [rows, 64] or NULL; backward only                                                          */
    float* grad_weight;                 /* [1, 64] or NULL; backward only                                                             */
    float* grad_bias;                   /* [1] or NULL; backward only                                                                 */
    void* workspace;                    /* gmpe_value_workspace_bytes(rows, 1) bytes, 8-byte aligned; backward only                   */
    size_t workspace_bytes;
} gmpe_value_plan;
/* want_backward == 0: 0 bytes. */
int gmpe_value_workspace_bytes(int64_t rows, int32_t want_backward, size_t* bytes_out);
int gmpe_value_forward(int device, const gmpe_value_plan* plan, void* stream);
int gmpe_value_backward(int device, const gmpe_value_plan* plan, void* stream);

/* ---- The gradient clip and the Adam step of GR_MAPPO.ppo_update (handle-less) ----
 * nn.utils.clip_grad_norm_ followed by torch.optim.Adam.step (onpolicy/algorithms/graph_mappo.py:212-227 and :254-265) over a table of float32 tensors:
 * the 2-norm of the gradients flagged GMPE_OPT_T_IN_NORM, those gradients scaled by the clip coefficient, and torch's single-tensor Adam on the tensors
 * flagged GMPE_OPT_T_STEP. The two sets may differ (after a PopArt update that installs new Parameters the reference clips critic.parameters() and steps
 * the optimiser's own list). All arrays contiguous, 4-byte aligned (views at odd float offsets are fine: every access is one dword), none overlapping
 * another; a tensor appears once in the table. Tensors with numel == 0 are skipped. Everything the host can see is checked before any launch; a refusal
 * is GMPE_ERR_INVALID_ARG with the function and the field in gmpe_last_error.
 *
 * Geometry. The tensors with numel > 0 are cut, in table order, into launch groups: a group ends before the tensor that would be its
 * (GMPE_OPT_MAX_TENSORS + 1)-th, that would bring a (GMPE_OPT_MAX_HYPERS + 1)-th distinct `hyper` index into it, or that would take its elements past
 * 2^31 - 1 - GMPE_OPT_CHUNK. A group's elements are concatenated in table order and cut into chunks of GMPE_OPT_CHUNK elements, one workgroup of 256
 * threads per chunk (thread i owns elements i, i + 256, i + 512, i + 768 of its chunk); the group's table (pointers, prefix sums, flags, and the float32
 * hyper-parameters) travels as kernel arguments, so nothing is uploaded, allocated or cached between calls: gradient addresses may change every call.
 * The chunks of all groups are numbered in group order: n_chunks = sum over groups of ceil(group elements / GMPE_OPT_CHUNK).
 *
 * Launches on `stream`, 2 per group, every group's k_opt_norm before any group's k_opt_step (a table without elements: one k_opt_step that writes `out`):
 *   k_opt_norm   part[c] = the sum over chunk c of (double)g * (double)g for the elements of GMPE_OPT_T_IN_NORM tensors (exact products; 0 for the
 *                others): each thread adds its four in ascending order, then the 256 sums are added pairwise by halving (i += i + 128, then + 64, ..., + 1).
 *   k_opt_step   every workgroup forms total = sum of part[0 .. n_chunks) itself — thread i adds part[i], part[i + 256], ... ascending, then the same
 *                halving — so every workgroup holds the same bits, a function of the shapes, the flags and the data. No atomics.
 *     total_norm = sqrt(total)                                                            (double)
 *     coef       = (float)min(1.0, max_norm / (total_norm + 1e-6))                        formed in double, rounded once; NaN stays NaN; GMPE_OPT_CLIP only
 *     out[0] = total_norm, out[1] = coef (1.0 without GMPE_OPT_CLIP), grad_norm_f32[0] = (float)total_norm: written by the first workgroup
 *     per element of a GMPE_OPT_T_IN_NORM tensor, GMPE_OPT_CLIP only:   g = g * coef, written back to grad (also when coef == 1, as torch multiplies)
 *     per element of a GMPE_OPT_T_STEP tensor, GMPE_OPT_STEP only, all float32, no fused multiply-add, g as it stands after the clip (the gradient of a
 *     tensor that is not GMPE_OPT_T_IN_NORM is used unscaled; the decayed g is not written back):
 *       g     = g + wd * p                       when wd != 0
 *       m     = m + (g - m) * w1                 w1 = (float)(1 - beta1)                  exp_avg.lerp_(grad, 1 - beta1)
 *       v     = b2 * v + (w2 * g) * g            b2 = (float)beta2, w2 = (float)(1 - beta2)   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
 *       denom = sqrtf(v) / s2 + eps              s2 = (float)sqrt(1 - beta2^t)            correctly rounded sqrt and divide
 *       p     = p - a * (m / denom)              a  = (float)(lr / (1 - beta1^t))         param.addcdiv_(exp_avg, denom, value=-step_size)
 *     The host forms w1, w2, a and s2 in double from the plan's doubles and t and rounds each to float32 once, as a Python float is when it meets a
 *     float32 tensor. Non-finite values propagate as the formulas say and nothing is skipped: an infinite gradient entry gives total_norm = inf and
 *     coef = 0, so that entry becomes NaN and the other clipped gradients 0.
 * Two calls from the same state give the same bits. Workspace: f64 part[n_chunks]; its contents before the call do not matter. */
#define GMPE_OPT_MAX_TENSORS 64        /* tensors per launch group                                                                      */
#define GMPE_OPT_MAX_HYPERS 8          /* distinct hyper-parameter sets per launch group                                                 */
#define GMPE_OPT_CHUNK 1024            /* elements per workgroup: 256 threads x 4 dwords, every access coalesced                          */
#define GMPE_OPT_MAX_PLAN_TENSORS 4096 /* tensors per call                                                                               */
#define GMPE_OPT_MAX_NUMEL (1LL << 30) /* elements per tensor                                                                            */
#define GMPE_OPT_CLIP 1                /* plan flag: scale the GMPE_OPT_T_IN_NORM gradients by coef                                       */
#define GMPE_OPT_STEP 2                /* plan flag: step the GMPE_OPT_T_STEP tensors                                                     */
#define GMPE_OPT_T_IN_NORM 1           /* tensor flag: its gradient enters the norm and is scaled                                         */
#define GMPE_OPT_T_STEP 2              /* tensor flag: Adam steps it, with hypers[hyper]                                                  */
typedef struct gmpe_optim_tensor {
    float* param;                       /* [numel]; read and written with GMPE_OPT_T_STEP, else not read (may be NULL)                 */
    float* grad;                        /* [numel]; required                                                                           */
    float* exp_avg;                     /* [numel]; GMPE_OPT_T_STEP                                                                    */
    float* exp_avg_sq;                  /* [numel]; GMPE_OPT_T_STEP                                                                    */
    int64_t numel;                      /* 0 .. GMPE_OPT_MAX_NUMEL; 0: the tensor is skipped                                           */
    int32_t flags;                      /* GMPE_OPT_T_*, at least one                                                                  */
    int32_t hyper;                      /* index into hypers with GMPE_OPT_T_STEP, else 0                                              */
} gmpe_optim_tensor;
typedef struct gmpe_optim_hyper {       /* one torch param_group at one step count                                                     */
    double lr;                          /* >= 0                                                                                        */
    double beta1, beta2;                /* in [0, 1)                                                                                   */
    double eps;                         /* >= 0                                                                                        */
    double weight_decay;                /* >= 0 (torch's coupled weight decay: added to the gradient)                                  */
    int64_t t;                          /* the step count AFTER this step, >= 1                                                        */
} gmpe_optim_hyper;
typedef struct gmpe_optim_plan {
    int32_t n_tensors;                  /* 1 .. GMPE_OPT_MAX_PLAN_TENSORS                                                              */
    int32_t n_hypers;                   /* 0 .. GMPE_OPT_MAX_PLAN_TENSORS                                                              */
    int32_t flags;                      /* GMPE_OPT_CLIP | GMPE_OPT_STEP, or 0: the norm is only reported                              */
    int32_t reserved;                   /* 0                                                                                           */
    const gmpe_optim_tensor* tensors;   /* HOST array [n_tensors]                                                                      */
    const gmpe_optim_hyper* hypers;     /* HOST array [n_hypers]                                                                       */
    double max_norm;                    /* > 0 with GMPE_OPT_CLIP (inf allowed), else not read                                         */
    double* out;                        /* f64 [2] device: total_norm, coef; 8-byte aligned                                            */
    float* grad_norm_f32;               /* f32 [1] device or NULL: total_norm rounded once                                             */
    void* workspace;                    /* gmpe_optim_workspace_bytes(plan) bytes, 8-byte aligned; may be NULL when that is 0          */
    size_t workspace_bytes;
} gmpe_optim_plan;
/* bytes of workspace for this plan's geometry: reads n_tensors, n_hypers and the tensors' numel, flags and hyper; no pointer into device memory */
int gmpe_optim_workspace_bytes(const gmpe_optim_plan* plan, size_t* bytes_out);
int gmpe_optim_step(int device, const gmpe_optim_plan* plan, void* stream);

/* The same call for a learner whose minibatch lies in `world` shards (see gmpe_compute_returns_shard, gmpe_ppo_loss_shard): every shard has run its own
 * backward over its own rows, and the clip and the step work on the SUM over the shards of their gradients — a sum, not a mean: it pairs with
 * gmpe_ppo_loss_shard, whose shards' gradients add up to the gradient of the whole minibatch. Two phases around one exchange the caller makes, an
 * all-gather of `local` into `all` (row r = shard r). The tables of all shards must be equal: the same tensors with numel > 0, in the same order.
 *   GMPE_SHARD_LOCAL  k_opt_pack, one launch per group: the gradients of every tensor of the table, GMPE_OPT_T_IN_NORM or GMPE_OPT_T_STEP, copied back to
 *                     back in table order into local[0 .. n), n = gmpe_optim_shard_elems(&base). It reads the geometry and the `grad` pointers of
 *                     `base` and nothing else (param, exp_avg, exp_avg_sq, hypers' values, out, workspace may still be unset), and writes only `local`.
 *   GMPE_SHARD_APPLY  two launches per group, every group's k_opt_reduce before any group's k_opt_step:
 *     k_opt_reduce    in place of k_opt_norm. Per element e of the packed order
 *                         g = (float)( ((double)all[0 * n + e] + (double)all[1 * n + e]) + ... + (double)all[(world - 1) * n + e] )
 *                     a left fold in shard order that starts at shard 0's value, in double, rounded once (the loads of up to 8 shards are issued before
 *                     their adds). g is written to the tensor's own grad, so the gradients hold the global gradient afterwards, on every shard the
 *                     same bits; part[c] = the sum over chunk c of (double)g * (double)g over the GMPE_OPT_T_IN_NORM elements, in k_opt_norm's layout
 *                     and order.
 *     k_opt_step      as in gmpe_optim_step, line by line: the norm, the coefficient, the clip of the summed gradient, and Adam on it.
 *                     APPLY checks `base` as gmpe_optim_step does.
 * With world = 1 and all == local, LOCAL then APPLY is gmpe_optim_step bit for bit. Because every shard adds the same rows in the same order, parameters,
 * Adam state and the norm stay bit-identical across replicas; an all-reduce, whose order belongs to its backend, would not promise that. Non-finite
 * values propagate: a NaN in one shard's gradient is a NaN in every shard's sum. Neither phase allocates, uses atomics or waits for the device.
 * Refused before any device call, beyond what `base` is refused for: a null plan, an unknown phase, world outside 1 .. GMPE_SHARD_MAX_WORLD, a missing
 * or misaligned `local` (LOCAL) or `all` (APPLY), local_elems != gmpe_optim_shard_elems(&base), world * local_elems > 2^31 - 1. */
typedef struct gmpe_optim_shard_plan {
    gmpe_optim_plan base;               /* as for gmpe_optim_step                                                                      */
    int32_t phase;                      /* GMPE_SHARD_LOCAL or GMPE_SHARD_APPLY                                                        */
    int32_t world;                      /* shards, 1 .. GMPE_SHARD_MAX_WORLD                                                           */
    float* local;                       /* f32 [local_elems] device, 4-byte aligned: written by LOCAL (not read by APPLY)              */
    const float* all;                   /* f32 [world, local_elems] device, 4-byte aligned: read by APPLY (not read by LOCAL)          */
    int64_t local_elems;                /* gmpe_optim_shard_elems(&base)                                                               */
} gmpe_optim_shard_plan;
/* the elements of `local`: the sum of the tensors' numel; reads what gmpe_optim_workspace_bytes reads */
int gmpe_optim_shard_elems(const gmpe_optim_plan* plan, int64_t* elems_out);
int gmpe_optim_step_shard(int device, const gmpe_optim_shard_plan* plan, void* stream);

/* The same call with Adam's step count in device memory, so that a captured graph (hipGraph) of it can be replayed: gmpe_optim_step forms a = lr /
 * (1 - beta1^t) and s2 = sqrt(1 - beta2^t) on the host from hypers[i].t and passes them as kernel arguments, which a replay would repeat for ever. Here
 * the float32 sets of `rows` consecutive step counts lie in device memory (the schedule), a device counter says which row the next call uses, and the
 * call's last launch advances it.
 *
 * The schedule. base's tensors are cut into launch groups as for gmpe_optim_step; a group's distinct `hyper` indices take its slots 0, 1, ... in the
 * order in which its GMPE_OPT_T_STEP tensors first name them. A slot is GMPE_OPT_HYPER_FLOATS float32: wd, w1, b2, w2, a, s2, eps of gmpe_optim_step's
 * formulas. A row is n_groups * GMPE_OPT_MAX_HYPERS slots — the row stride is n_groups * GMPE_OPT_MAX_HYPERS * GMPE_OPT_HYPER_FLOATS floats —, slot s
 * of group g at float (g * GMPE_OPT_MAX_HYPERS + s) * GMPE_OPT_HYPER_FLOATS of its row; slots not in use are 0. Row k holds every slot's set for the
 * step count hypers[i].t + k, so row 0 is what gmpe_optim_step would use for the same plan: one host function rounds the doubles for both, which makes
 * a scheduled step's bits gmpe_optim_step's. gmpe_optim_schedule_bytes gives rows * row stride * 4; gmpe_optim_schedule_fill writes the rows into HOST
 * memory (the caller uploads them; neither makes a device call; they read base's geometry, and fill the hypers' values, checked as gmpe_optim_step
 * checks them, and no pointer into device memory).
 *
 * gmpe_optim_step_scheduled launches on `stream`: every group's k_opt_norm as in gmpe_optim_step; every group's k_opt_step, which reads row = *counter
 * and takes its sets from schedule[row] instead of the kernel arguments, line by line the same arithmetic; then k_opt_advance, one thread, ++*counter.
 * Ordering: all on the one stream and the advance last, so every kernel of a call reads the counter before that call writes it, and the next call (or
 * the next replay) reads it after. hypers[i].t of `base` is not read by the launches (it is checked, >= 1): the device counter alone selects the row,
 * and the kernel arguments are the same at every call, which is what makes the call capturable.
 * Exhaustion: with *counter outside 0 .. rows - 1 no parameter, moment or gradient is touched (the clip included), *status becomes 1 and stays so
 * (nothing here ever clears it), the counter does not advance, and out and grad_norm_f32 still receive the norm and the coefficient.
 * No allocation, no atomics, no wait. Refused before any device call, beyond what `base` is refused for by gmpe_optim_step: a null plan, rows outside
 * 1 .. GMPE_OPT_MAX_SCHEDULE_ROWS, reserved != 0, GMPE_OPT_STEP without a schedule, a misaligned schedule, a missing or misaligned counter or status. */
#define GMPE_OPT_HYPER_FLOATS 7               /* float32 per schedule slot: wd, w1, b2, w2, a, s2, eps                                  */
#define GMPE_OPT_MAX_SCHEDULE_ROWS (1 << 20)  /* rows per schedule                                                                    */
typedef struct gmpe_optim_sched_plan {
    gmpe_optim_plan base;               /* as for gmpe_optim_step                                                                      */
    const float* schedule;              /* f32 [rows][row stride] device, 4-byte aligned: gmpe_optim_schedule_fill's rows; required with GMPE_OPT_STEP */
    int32_t* counter;                   /* i32 [1] device: the row the next call uses; read by every k_opt_step, advanced by the last launch */
    int32_t* status;                    /* i32 [1] device, sticky: set to 1 by a call past the schedule, never cleared                 */
    int32_t rows;                       /* 1 .. GMPE_OPT_MAX_SCHEDULE_ROWS                                                             */
    int32_t reserved;                   /* 0                                                                                           */
} gmpe_optim_sched_plan;
int gmpe_optim_schedule_bytes(const gmpe_optim_plan* plan, int32_t rows, size_t* bytes_out);
int gmpe_optim_schedule_fill(const gmpe_optim_plan* plan, int32_t rows, void* host_dst);
int gmpe_optim_step_scheduled(int device, const gmpe_optim_sched_plan* plan, void* stream);

/* ---- The policy's masked GRU layer (handle-less): RNNLayer.forward (onpolicy/algorithms/utils/rnn.py:23-79) with recurrent_N == 1 ----
 * The layer in front of the action head (GR_Actor) and of the value head (GR_Critic): nn.GRU(D, H) driven step by step with the state multiplied by
 * the step's mask, then nn.LayerNorm(H). All arrays float32, contiguous. For every row k of `rows` independently, t = 0 .. steps-1 (x, masks, features
 * and grad_* of the [steps * rows] arrays are time-major: row t * rows + k):
 *     h <- h * masks[t, k]
 *     r = sigmoid(W_ir x_t + b_ir + W_hr h + b_hr),  z = sigmoid(W_iz x_t + b_iz + W_hz h + b_hz),  n = tanh(W_in x_t + b_in + r * (W_hn h + b_hn))
 *     h <- (1 - z) * n + z * h
 *     features[t, k] = LayerNorm(h)            biased variance, eps inside the square root
 * and hxs_out[k] = the last h, not normalised. For masks in {0, 1} this is the reference's segment loop (it splits the sequence at every step at which
 * ANY row has a zero and multiplies every row by its own mask there; a row whose mask is 1 is untouched) and, with steps == 1, its rollout branch.
 * Masks outside {0, 1} are undefined here (in the reference their effect depends on the other rows of the batch) and are not checked.
 * Supported: in_dim == hidden == 64 (every shipped checkpoint); anything else is refused before any launch.
 * Arithmetic of one row (float32, a function of (in_dim, hidden) alone — not of steps, rows, the row's place in a tile or its neighbours): every
 * pre-activation is one fmaf chain in ascending k, r and z from b_i + b_h over x then over h, the two n terms from b_in over x and from b_hn over h;
 * sigmoid = 1 / (1 + expf(-a)), tanhf; the LayerNorm sums are xor trees over the 64 columns (offsets 32, 16, .. 1).
 * gmpe_gru_forward: ONE launch. With a workspace (a training plan) it keeps r, z, n, W_hn h + b_hn, h and the LayerNorm mean / rstd of every (t, k) in
 * it; with workspace == NULL (the rollout step, under no_grad) it writes nothing but features and hxs_out, and the gradient pointers may be NULL.
 * hxs_out may be hxs itself in a forward-only plan; any other overlap of hxs_out with an input, a parameter, features or the workspace is refused.
 * gmpe_gru_backward (after gmpe_gru_forward on the same plan's inputs and workspace; may be repeated): THREE launches whatever steps, rows and masks.
 *   1 back-propagation through time, per tile of GMPE_GRU_ROW_TILE rows, t descending: LayerNorm backward, the gate gradients (kept in the workspace),
 *     grad_x[t, k] and the state gradient, multiplied by masks[t, k] on its way to step t-1 — so nothing flows across a step whose mask is 0 and
 *     grad_hxs of a row with masks[0] == 0 is 0; and the tile's double sums of the bias and LayerNorm gradients (t descending, the rows of a wave
 *     ascending, then the four waves in wave order);
 *   2 the weight gradients as double sums of exact products over P = min(128, ceil(steps * rows / 32)) contiguous parts of the steps * rows rows, in
 *     ascending row order inside a part;
 *   3 the parts added in ascending part order (weights), the tiles as 16 interleaved slices in ascending order and the slices in slice order (biases,
 *     LayerNorm), each rounded to float32 once.
 *   So a parameter gradient's summation order is a function of (steps, rows) alone. grad_hxs_out == NULL stands for zeros.
 * No atomics, no allocation, no host synchronisation; capturable. */
#define GMPE_GRU_ROW_TILE 32
typedef struct gmpe_gru_plan {
    int64_t steps;                      /* L >= 1                                                                                     */
    int64_t rows;                       /* Nb >= 1: the rows of hxs (chunks of a recurrent minibatch, or N*A of a rollout step)       */
    int32_t in_dim;                     /* D = 64                                                                                     */
    int32_t hidden;                     /* H = 64                                                                                     */
    double eps;                         /* LayerNorm.eps > 0                                                                          */
    const float* x;                     /* [steps * rows, D]                                                                          */
    const float* hxs;                   /* [rows, H] (the [rows, 1, H] state)                                                         */
    const float* masks;                 /* [steps * rows]                                                                             */
    const float* weight_ih;             /* [3H, D] gate order r, z, n                                                                 */
    const float* weight_hh;             /* [3H, H]                                                                                    */
    const float* bias_ih;               /* [3H]                                                                                       */
    const float* bias_hh;               /* [3H]                                                                                       */
    const float* ln_weight;             /* [H]                                                                                        */
    const float* ln_bias;               /* [H]                                                                                        */
    float* features;                    /* [steps * rows, H]                                                                          */
    float* hxs_out;                     /* [rows, H]                                                                                  */
    const float* grad_features;         /* [steps * rows, H]; backward                                                                */
    const float* grad_hxs_out;          /* [rows, H] or NULL (zeros); backward                                                        */
    float* grad_x;                      /* [steps * rows, D]; backward, like every grad_* below                                       */
    float* grad_hxs;                    /* [rows, H]                                                                                  */
    float* grad_weight_ih;              /* [3H, D]                                                                                    */
    float* grad_weight_hh;              /* [3H, H]                                                                                    */
    float* grad_bias_ih;                /* [3H]                                                                                       */
    float* grad_bias_hh;                /* [3H]                                                                                       */
    float* grad_ln_weight;              /* [H]                                                                                        */
    float* grad_ln_bias;                /* [H]                                                                                        */
    void* workspace;                    /* gmpe_gru_workspace_bytes(steps, rows, hidden, 1) bytes, 8-byte aligned; NULL: forward only */
    size_t workspace_bytes;
} gmpe_gru_plan;
/* want_backward == 0: 0 bytes (the forward-only plan takes no workspace). */
int gmpe_gru_workspace_bytes(int64_t steps, int64_t rows, int32_t hidden, int32_t want_backward, size_t* bytes_out);
int gmpe_gru_forward(int device, const gmpe_gru_plan* plan, void* stream);
int gmpe_gru_backward(int device, const gmpe_gru_plan* plan, void* stream);

/* ---- The policy's MLPBase (handle-less): MLPBase.forward (onpolicy/algorithms/utils/mlp.py:44-76), the stage in front of the GRU layer ----
 * GR_Actor runs it on torch.cat([obs, nbd_features]), GR_Critic on nbd_features or torch.cat([cent_obs, nbd_features]). Here the input is n_parts
 * (1 .. GMPE_MLP_MAX_PARTS) float32 arrays part[i] of [rows, part_dim[i]], contiguous, whose columns are read as if concatenated: D = sum of part_dim,
 * 1 <= D <= GMPE_MLP_MAX_IN. The concatenation is never written anywhere, and every part has a gradient array of its own. For every row independently:
 *     x <- LayerNorm_D(x)                          if feature_norm (fn_weight, fn_bias [D], fn_eps); biased variance, eps inside the square root
 *     x <- LayerNorm_64(act(W_l x + b_l))          for l = 0 .. layer_n: layer[0].weight is [64, D], layer[l > 0].weight [64, 64]; act = ReLU or Tanh
 *     features = x                                 [rows, 64]
 * Supported: hidden == 64, layer_n in 0 .. 2, float32; anything else is refused before any launch, with the field named.
 * Arithmetic of one row (a function of (D, layer_n, activation, feature_norm) alone — not of rows, of the row's place, of how the columns are split into
 * parts): every dot product is one fmaf chain from the bias in ascending k (layer 0 over D rounded up to a multiple of 4, the padding being zeros); every
 * other operation is rounded on its own; a LayerNorm sum is an xor tree over the 64 lanes (offsets 32, 16, .. 1), mean and variance multiplied by 1 / 64,
 * rstd = 1 / sqrt(var + eps). The feature norm's statistics are formed in double (lane j adds its columns j, j + 64, .. ascending, then the xor tree;
 * mean, (x - mean), the variance / D and rstd in double; (x - mean) * rstd rounded to float32 once): a row of 2 or 3 observations that lie close together
 * would lose in x - mean the digits a float32 mean does not have.
 * D == 1 with feature_norm is legal and degenerate: the normalised input is 0 for every row.
 * gmpe_mlp_forward: ONE launch; it reads the parts and the parameters, writes features, and neither reads nor writes the workspace: the forward-only plan
 * (workspace == NULL, gradient pointers NULL) and the training plan run the same kernel and give the same bits.
 * gmpe_mlp_backward (may be repeated; it needs no gmpe_mlp_forward before it — it recomputes a tile's forward, the same code and bits): THREE launches
 * whatever rows, D, layer_n and n_parts.
 *   1 per tile of GMPE_MLP_ROW_TILE rows: forward again, then LayerNorm, activation and Linear backward layer by layer and the feature norm's backward;
 *     grad_part[i] written; the workgroup's double sums of the bias, LayerNorm and feature-norm gradients (its tiles ascending, a wave's rows ascending,
 *     then the four waves in wave order);
 *   2 the weight gradients as double sums of exact products over P = min(128, ceil(rows / 32)) contiguous parts of the rows, ascending inside a part;
 *   3 the parts added in ascending order (weights), the workgroups of launch 1 as 16 interleaved slices in ascending order and the slices in slice order
 *     (everything else), each rounded to float32 once. So a parameter gradient's summation order is a function of (rows, D, layer_n) alone.
 * Workspace (training only; gmpe_mlp_workspace_bytes is the single source of its size; its contents before the call do not matter), in this order:
 *     double partC[G][(3 * 3 + 2 * 4) * 64]      G = the workgroups of launch 1: column (3 l + {0 bias, 1 ln_weight, 2 ln_bias}) * 64 + j, then fn_weight, fn_bias
 *     double partW[P][ceil(D / 64) + layer_n][64][64]
 *     double stats[rows][2]                      the feature norm's mean and rstd
 *     float  dpre[layer_n + 1][rows][64]         the gradients of the pre-activations
 *     float  out[layer_n][rows][64]              the outputs of layers 0 .. layer_n - 1 (the inputs of the hidden layers' weight gradients)
 * Outputs must not overlap inputs. No atomics, no allocation, no host synchronisation; capturable. */
#define GMPE_MLP_ROW_TILE 32
#define GMPE_MLP_MAX_PARTS 4
#define GMPE_MLP_MAX_IN 256
#define GMPE_MLP_MAX_LAYERS 3           /* fc1 and layer_n <= 2 copies of fc_h                                                        */
#define GMPE_MLP_RELU 0
#define GMPE_MLP_TANH 1
typedef struct gmpe_mlp_layer {
    const float* weight;                /* [64, D] (layer 0) or [64, 64]                                                              */
    const float* bias;                  /* [64]                                                                                       */
    const float* ln_weight;             /* [64]                                                                                       */
    const float* ln_bias;               /* [64]                                                                                       */
    double eps;                         /* this LayerNorm's eps > 0                                                                   */
    float* grad_weight;                 /* backward, like every grad_* here                                                           */
    float* grad_bias;
    float* grad_ln_weight;
    float* grad_ln_bias;
} gmpe_mlp_layer;
typedef struct gmpe_mlp_plan {
    int64_t rows;                       /* >= 1                                                                                       */
    int32_t hidden;                     /* 64                                                                                         */
    int32_t layer_n;                    /* 0 .. 2: MLPLayer._layer_N                                                                  */
    int32_t activation;                 /* GMPE_MLP_RELU or GMPE_MLP_TANH                                                             */
    int32_t feature_norm;               /* 0 or 1: MLPBase._use_feature_normalization                                                 */
    int32_t n_parts;                    /* 1 .. GMPE_MLP_MAX_PARTS                                                                    */
    int32_t reserved;
    const float* part[GMPE_MLP_MAX_PARTS];      /* [rows, part_dim[i]]                                                                */
    int32_t part_dim[GMPE_MLP_MAX_PARTS];       /* >= 1, their sum D <= GMPE_MLP_MAX_IN                                               */
    float* grad_part[GMPE_MLP_MAX_PARTS];       /* [rows, part_dim[i]]; backward                                                      */
    const float* fn_weight;             /* [D]; with feature_norm, like the four fields below                                         */
    const float* fn_bias;               /* [D]                                                                                        */
    double fn_eps;                      /* > 0                                                                                        */
    float* grad_fn_weight;              /* [D]; backward                                                                              */
    float* grad_fn_bias;                /* [D]; backward                                                                              */
    gmpe_mlp_layer layer[GMPE_MLP_MAX_LAYERS];  /* layer[0 .. layer_n] are read                                                       */
    float* features;                    /* [rows, 64]; forward (backward does not need it)                                            */
    const float* grad_features;         /* [rows, 64]; backward                                                                       */
    void* workspace;                    /* gmpe_mlp_workspace_bytes(rows, D, hidden, layer_n, 1) bytes, 8-byte aligned; backward only */
    size_t workspace_bytes;
} gmpe_mlp_plan;
/* want_backward == 0: 0 bytes (the forward-only plan takes no workspace). */
int gmpe_mlp_workspace_bytes(int64_t rows, int32_t in_dim, int32_t hidden, int32_t layer_n, int32_t want_backward, size_t* bytes_out);
int gmpe_mlp_forward(int device, const gmpe_mlp_plan* plan, void* stream);
int gmpe_mlp_backward(int device, const gmpe_mlp_plan* plan, void* stream);

/* ---- The policy's GNNBase (handle-less): GNNBase.forward (onpolicy/algorithms/utils/gnn_new.py:492-510), the first stage of GR_Actor / GR_Critic ----
 * One module per call: nbd_features [rows, 16] from node_obs [rows, E, F], the dense adjacency and agent_id [rows]. Row g is one graph of E nodes.
 *   edges      j -> i exists iff 0 < adj[j, i] < max_edge_dist (float32 compares, strict), e = adj[j, i]; the matrix is read as it is (no symmetry assumed)
 *              and no edge list is ever built. adj is [rows / adj_share, E, E]: matrix g / adj_share serves row g (adj_share = 1: one matrix per row;
 *              adj_share = A: the compact adjacency of a rollout step). rows must be a multiple of adj_share; the result has the bits of the materialised form.
 *   EmbedConv  per edge m = [x_j[0 .. F-2], entity_embed[int(x_j[F-1])], e]; y = LN(act(lin1 m)); embed_layer_n times y = LN(act(W_l y + b_l)) with the SAME
 *              LayerNorm parameters (embed_layer_norm = 0: no LayerNorm at all); x_i = sum over the incoming edges of i (none: zeros).
 *              An entity type outside [0, num_embeddings) is clamped into it, and that row's value is then unspecified; nothing is read out of bounds.
 *   conv[0 .. gnn_layer_n] (TransformerConv, heads H of 16 channels, averaged, no beta, no dropout): q, k, v = lin_query / lin_key / lin_value (x) as
 *              [E, H, 16]; ee = lin_edge_weight * e; alpha_ji = softmax over the incoming edges of i of q_i . (k_j + ee_ji) / 4;
 *              out_i = (sum over heads of sum_j alpha_ji (v_j + ee_ji)) / H + lin_skip(x_i); x = act(out). A node without incoming edge keeps the skip term.
 *   output     GMPE_GNN_NODE: the row of node agent_id[g] (clamped into [0, E): a bad id reads nothing out of bounds, its row is unspecified);
 *              GMPE_GNN_MEAN / _MAX / _ADD: the pool over all E nodes, isolated ones included.
 * Supported: float32, hidden == 16, heads 1 .. 4, gnn_layer_n 0 .. 2, embed_layer_n 0 .. 2, edge_dim == 1, 2 <= F <= 16, num_embeddings 1 .. 16,
 * embedding_size 1 .. 8, 1 <= E <= 64, concat == 0, beta == 0. Anything else is refused before any launch, with the field named.
 * Arithmetic of one graph (a function of E and the configuration alone — not of rows, of the graph's place in the call, of adj_share). One lane owns one
 * node; every sum over nodes or edges runs in ascending node index; contraction is off and every operation not named here is rounded on its own.
 *   P_j   = fmaf chain from lin1_bias over lin1_weight[:, k] * m[k], k = 0 .. F + embedding_size - 2 ascending (the node's part of lin1);
 *   edge  pre = fmaf(lin1_weight[:, last], e, P_j); a = max(pre, 0) or float(tanh(double(pre))); LayerNorm over the 16 values with its statistics in
 *         double (sums ascending from 0, mean and variance times 1 / 16, rstd = 1 / sqrt(var + eps), (a - mean) * rstd rounded to float32 once), then
 *         xh * w + b in float32; a 16 x 16 Linear is an fmaf chain from the bias, k ascending; x_i = the double sum of the edges' outputs, j ascending
 *         from 0, rounded to float32 once;
 *   conv  logit = (fmaf chain from 0 over c of q_i[c] * fmaf(we[c], e, k_j[c])) * 0.25; m = max over j; p = expf(logit - m); s = sum of p (j ascending);
 *         acc[c] = fmaf chain over j of p * fmaf(we[c], e, v_j[c]); head = acc / s; heads added in ascending order from 0, divided by H, plus the skip
 *         Linear; the 1e-16 of the reference's softmax denominator is below one ulp of s >= 1 and is dropped;
 *   pools sums and maxima over i ascending; the mean is the sum divided by E.
 *   backward: every difference that cancels is formed in double from the float32 values of the forward and rounded once — the dot products dout . v of
 *         the softmax backward (exact products, c ascending), its own softmax (the sum of p in double, alpha = p / sum in double, so that the logit
 *         gradients of a target add up to zero to double precision), the LayerNorm's backward means; Tanh's derivative is (1 - y) (1 + y).
 * gmpe_gnn_forward: ONE launch; it reads the inputs and the parameters, writes features, and neither reads nor writes the workspace: the forward-only
 * plan (workspace == NULL, gradient pointers NULL) and the training plan run the same kernel and give the same bits.
 * gmpe_gnn_backward (may be repeated; it needs no gmpe_gnn_forward before it — it recomputes a graph's forward, the same code and bits): THREE launches
 * whatever rows, E and the data. The inputs get no gradient.
 *   1 a workgroup of 256 threads owns tiles of W graphs (W = 1 .. 4 graphs side by side, a function of E and the configuration: what fits the LDS),
 *     tile blockIdx.x, blockIdx.x + gridDim.x, ...: forward again, then the pool and the convs backward; the gradient of the EmbedConv's output is
 *     written to the workspace. A parameter-gradient element belongs to one thread of the workgroup. A tile's contribution to it is a double sum from 0
 *     of exact products over the tile's graphs in ascending order and a graph's nodes in ascending order (a per-edge term first summed over
 *     a source node's targets, ascending, in double, and rounded once when staged); it is added to the workgroup's running double sum. A conv's input
 *     gradient (the skip's and every head's three Linears, transposed) is one double sum of exact products, rounded to float32 once.
 *   2 the same tiles: the EmbedConv backward, every edge's MLP recomputed; its parameters' sums as in 1, the per-edge layers' once per target node.
 *   3 the workgroups' double sums added in ascending workgroup order and rounded to float32 once.
 *   So a parameter gradient's summation order is a function of (rows, E, configuration) alone, and two calls give the same bits.
 * Workspace (training only; gmpe_gnn_workspace_bytes is the single source of its size; its contents before the call do not matter):
 *     double part[G][NP]      G = min(ceil(rows / W), 256) workgroups of launches 1 and 2; NP = the parameters in the order entity_embed (rounded up to 4 floats),
 *                             lin1 weight, lin1 bias, LayerNorm weight, bias (16 + 16, reserved also without LayerNorm), (weight, bias) per embed layer,
 *                             then per conv (query weight, bias, key weight, bias, value weight, bias, edge weight, skip weight, bias)
 *     float  dX[rows][E][16]  the gradient of the EmbedConv's output, from launch 1 to launch 2
 * Outputs must not overlap inputs. No atomics, no allocation, no host synchronisation; capturable. */
#define GMPE_GNN_HIDDEN 16
#define GMPE_GNN_MAX_NODES 64
#define GMPE_GNN_MAX_HEADS 4
#define GMPE_GNN_MAX_CONVS 3            /* gnn1 and gnn_layer_n <= 2 of gnn2                                                          */
#define GMPE_GNN_MAX_EMBED_LAYERS 2
#define GMPE_GNN_MAX_FEATS 16
#define GMPE_GNN_MAX_EMBEDDINGS 16
#define GMPE_GNN_MAX_EMBEDDING_SIZE 8
#define GMPE_GNN_RELU 0
#define GMPE_GNN_TANH 1
#define GMPE_GNN_NODE 0
#define GMPE_GNN_MEAN 1
#define GMPE_GNN_MAX 2
#define GMPE_GNN_ADD 3
typedef struct gmpe_gnn_conv {          /* one TransformerConv; H = heads                                                             */
    const float* query_weight;          /* [16 H, 16]                                                                                 */
    const float* query_bias;            /* [16 H]                                                                                     */
    const float* key_weight;
    const float* key_bias;
    const float* value_weight;
    const float* value_bias;
    const float* edge_weight;           /* [16 H, 1], no bias                                                                         */
    const float* skip_weight;           /* [16, 16]                                                                                   */
    const float* skip_bias;             /* [16]                                                                                       */
    float* grad_query_weight;           /* backward, like every grad_* here                                                           */
    float* grad_query_bias;
    float* grad_key_weight;
    float* grad_key_bias;
    float* grad_value_weight;
    float* grad_value_bias;
    float* grad_edge_weight;
    float* grad_skip_weight;
    float* grad_skip_bias;
} gmpe_gnn_conv;
typedef struct gmpe_gnn_plan {
    int64_t rows;                       /* >= 1, a multiple of adj_share                                                              */
    int32_t num_nodes;                  /* E: 1 .. 64                                                                                 */
    int32_t node_feats;                 /* F: 2 .. 16, the last column is the entity type                                             */
    int32_t adj_share;                  /* >= 1: consecutive rows served by one adjacency matrix                                      */
    int32_t hidden;                     /* 16: embed_hidden_size and gnn_hidden_size                                                  */
    int32_t heads;                      /* 1 .. 4                                                                                     */
    int32_t concat;                     /* 0                                                                                          */
    int32_t beta;                       /* 0                                                                                          */
    int32_t edge_dim;                   /* 1                                                                                          */
    int32_t gnn_layer_n;                /* 0 .. 2                                                                                     */
    int32_t embed_layer_n;              /* 0 .. 2                                                                                     */
    int32_t embed_activation;           /* GMPE_GNN_RELU or GMPE_GNN_TANH                                                             */
    int32_t conv_activation;
    int32_t embed_layer_norm;           /* 0 or 1                                                                                     */
    int32_t aggregate;                  /* GMPE_GNN_NODE, _MEAN, _MAX or _ADD                                                         */
    int32_t num_embeddings;             /* 1 .. 16                                                                                    */
    int32_t embedding_size;             /* 1 .. 8                                                                                     */
    double max_edge_dist;               /* compared as float32                                                                        */
    double ln_eps;                      /* > 0 with embed_layer_norm                                                                  */
    const float* node_obs;              /* [rows, E, F]                                                                               */
    const float* adj;                   /* [rows / adj_share, E, E]                                                                   */
    const int32_t* agent_id;            /* [rows]; read with GMPE_GNN_NODE only                                                       */
    const float* entity_embed;          /* [num_embeddings, embedding_size]                                                           */
    const float* lin1_weight;           /* [16, F - 1 + embedding_size + 1]                                                           */
    const float* lin1_bias;             /* [16]                                                                                       */
    const float* ln_weight;             /* [16]; with embed_layer_norm, like ln_bias and their gradients                              */
    const float* ln_bias;
    const float* embed_weight[GMPE_GNN_MAX_EMBED_LAYERS];       /* [16, 16]                                                           */
    const float* embed_bias[GMPE_GNN_MAX_EMBED_LAYERS];         /* [16]                                                               */
    float* grad_entity_embed;
    float* grad_lin1_weight;
    float* grad_lin1_bias;
    float* grad_ln_weight;              /* the sum over every use of the one LayerNorm                                                */
    float* grad_ln_bias;
    float* grad_embed_weight[GMPE_GNN_MAX_EMBED_LAYERS];
    float* grad_embed_bias[GMPE_GNN_MAX_EMBED_LAYERS];
    gmpe_gnn_conv conv[GMPE_GNN_MAX_CONVS];                     /* conv[0 .. gnn_layer_n] are read                                    */
    float* features;                    /* [rows, 16]; forward (backward does not need it)                                            */
    const float* grad_features;         /* [rows, 16]; backward                                                                       */
    void* workspace;                    /* gmpe_gnn_workspace_bytes(plan, 1) bytes, 8-byte aligned; backward only                     */
    size_t workspace_bytes;
} gmpe_gnn_plan;
/* The size depends on rows, num_nodes, node_feats, heads, gnn_layer_n, embed_layer_n, num_embeddings and embedding_size only (no pointer is read).
 * want_backward == 0: 0 bytes (the forward-only plan takes no workspace). */
int gmpe_gnn_workspace_bytes(const gmpe_gnn_plan* plan, int32_t want_backward, size_t* bytes_out);
int gmpe_gnn_forward(int device, const gmpe_gnn_plan* plan, void* stream);
int gmpe_gnn_backward(int device, const gmpe_gnn_plan* plan, void* stream);

/* ---- The same GNNBase straight from the fp64 entity table (gmpe_outputs.entity_table): the policy as a consumer of the table form ----
 * Graph g is the view of ego = agent_id[g] of table row idx: idx = table_index[g] with an index, g / table_share without one (a rollout step's [N, W]
 * table serves its N * A rows with table_share = A). Nothing else changes: the plan wraps an unchanged gmpe_gnn_plan, and
 *     features, gradients == gmpe_gnn_forward / _backward on node_obs[g] = the row gmpe_expand_node_obs gives for (idx, ego), adj[g] = the matrix
 *     gmpe_expand_adj gives for idx, BIT FOR BIT
 * for equal base.rows (a parameter gradient's summation order is a function of (rows, E, configuration), as above). The kernels rebuild entry (j, i) of
 * the matrix and node `lane`'s row in the step that stages a graph's inputs in LDS, with the arithmetic those two entry points share, and everything
 * behind that step is the code of gmpe_gnn_forward / _backward: ONE launch forward, THREE backward, the same workspace (gmpe_gnn_workspace_bytes of
 * the base plan: the same function of the shapes), no atomics, no allocation, no host synchronisation, capturable. Neither [rows, E, F] nor [rows, E, E]
 * exists in memory: a graph costs its 4- or 8-byte index next to a table that is already there.
 * It is not faster: the GNN's arithmetic dominates, and every graph rebuilds its own E x E matrix (DESIGN.md 3.13 has the measured times). Its purpose is bytes.
 * base.node_obs, base.adj and base.adj_share are not read. base.num_nodes and base.node_feats must be gmpe_num_entities(cfg) and gmpe_node_feats(cfg).
 * base.agent_id is always required: the view needs its ego, whatever the aggregate. idx is clamped into [0, table_rows) and ego into [0, num_agents):
 * nothing is read out of bounds, and such a row's value is unspecified. Refused before any device call, with the function and the field named: a null
 * plan, cfg or table; num_nodes / node_feats that disagree with cfg; a table not 8-byte aligned; a table_index not 4-byte (index64 = 0) or 8-byte
 * (index64 = 1) aligned; table_rows < 1; without an index, table_share < 1 or rows not a multiple of it; and everything gmpe_gnn_forward refuses. */
typedef struct gmpe_gnn_table_plan {
    gmpe_gnn_plan base;                 /* as for gmpe_gnn_forward / _backward; node_obs, adj and adj_share are not read                */
    const gmpe_config* cfg;             /* host memory: the scenario, feature type and entity counts the table was written with          */
    const double* table;                /* [table_rows, W] f64 device memory, W = gmpe_entity_table_width(cfg), 8-byte aligned          */
    int64_t table_rows;                 /* >= 1                                                                                       */
    const void* table_index;            /* [rows] int32 or int64 device memory, or NULL: idx = g / table_share                        */
    int32_t index64;                    /* 0: table_index is int32; 1: int64                                                          */
    int32_t table_share;                /* without table_index: >= 1, rows a multiple of it; ignored with one                         */
} gmpe_gnn_table_plan;
int gmpe_gnn_forward_table(int device, const gmpe_gnn_table_plan* plan, void* stream);
int gmpe_gnn_backward_table(int device, const gmpe_gnn_table_plan* plan, void* stream);

/* ---- The same GNNBase's forward on graphs of up to 128 nodes: rollout, evaluation and the value bootstrap at more entities than 64 ----
 * gmpe_gnn_forward / gmpe_gnn_forward_table with num_nodes in 1 .. GMPE_GNN_WIDE_MAX_NODES (for the table form, cfg's entity count); every other
 * field, check and refusal is theirs, under these entries' names. Forward only: the gradient pointers, workspace and workspace_bytes are not read,
 * and there is no backward at num_nodes > 64 (gmpe_gnn_backward refuses it as before).
 *   num_nodes <= 64: the narrow entry's own launch — the bits are gmpe_gnn_forward's by construction, so a caller need not branch.
 *   num_nodes  > 64: one launch of a kernel in which a node belongs to a thread of a pair of waves, not to a lane of one wave. A workgroup of 256
 *     threads owns tiles of W graphs, W = 2 where two graphs' state fits 160 KiB of LDS next to the parameters and 1 above; pair p owns graph p of the
 *     tile, its thread t node t. The arithmetic of a graph is the one written above, a function of E and the configuration alone: every sum over a
 *     node's edges runs ascending in the node's thread, heads are added ascending, a pool adds the nodes ascending in one thread per channel. So a
 *     graph's row does not depend on rows, on its place in the call, on W, on adj_share or on the source, and appending isolated nodes (type 0, all
 *     their adjacency entries 0 or >= max_edge_dist) to a graph of <= 64 nodes leaves every original node's row at gmpe_gnn_forward's bits.
 * Every configuration gmpe_gnn_forward accepts fits at 128 nodes (162 816 B with 16 features, 4 heads, 3 convs, 2 embed layers, 16 x 8 embeddings).
 * gmpe_gnn_wide_geometry: the launch of a plan's shape (no pointer is read) -> out[0] = W (for num_nodes <= 64 the narrow forward's), out[1] = the
 * launch's dynamic LDS in bytes, out[2] = its workgroups. No atomics, no allocation, no host synchronisation; capturable. */
#define GMPE_GNN_WIDE_MAX_NODES 128
int gmpe_gnn_forward_wide(int device, const gmpe_gnn_plan* plan, void* stream);
int gmpe_gnn_forward_wide_table(int device, const gmpe_gnn_table_plan* plan, void* stream);
int gmpe_gnn_wide_geometry(const gmpe_gnn_plan* plan, int64_t* out);

/* ---- Evaluation of a policy over a batch of episodes (handle-less): GMPERunner.render(get_metrics=True) as one episode per env ----
 * (onpolicy/runner/shared/graph_mpe_runner.py:526-1060, base_runner.py:194-574). Every env plays one episode from a reset; the caller's policy acts,
 * the engine steps, gmpe_episode_record books the step. No allocation, no host synchronisation, every launch on `stream`.
 *
 * gmpe_episode_record, once per step t = 0 .. T-1 after the env step, same stream. For an env that is live:
 *   ret[n, a] += double(reward[n, a]) (the terminal step's reward counts); when every agent of env n is done or t == T-1 (the render loop's
 *   break on reset_count > 0, or the end of its range(episode_length)): final_info[n] = info[n], steps[n] = t + 1, live[n] = 0.
 * A finished env is frozen: the engine's auto-reset keeps stepping it and its later steps are ignored. Info rows are read only for envs that
 * finish at this step. The same launch writes what the policy acts with at step t + 1, for every env:
 *   masks f32 [N, A, 1]: 0 where done, all ones in an env whose agents are all done (:630-638);
 *   available_actions f32 [N, A, n_actions]: the one-hot stop row at n_actions / 2 where the mask is 0, else ones (:570-583);
 *   rnn_states f32 [N, A, rnn_row] (optional): the rows of done agents zeroed (:628). */
#define GMPE_EVAL_INFO_WIDTH 18          /* config.INFO_KEYS: 17 render keys + Phase_reached                                          */
#define GMPE_EVAL_NUM_COLUMNS 16         /* columns of gmpe_episode_metrics, in this order:                                           */
#define GMPE_EVAL_REWARD 0               /* mean over agents of ret (graph_mpe_runner.py:668)                                         */
#define GMPE_EVAL_FRAC 1                 /* max over agents of ttg / (T*dt) (np.any(list == 1) is always False there: :661-665)       */
#define GMPE_EVAL_SUCCESS 2              /* mean over agents of Dist_to_goal < min_dist_thresh (base_runner.py:499-505)              */
#define GMPE_EVAL_COLLISIONS 3           /* sum over agents, in agent order, of Num_agent_collisions / 2, then Num_obst_collisions     */
#define GMPE_EVAL_FAIRNESS 4             /* Mean_by_variance of agent A-1                                                             */
#define GMPE_EVAL_DIST_MEAN 5            /* Distance_mean of agent A-1                                                                */
#define GMPE_EVAL_TIME_MEAN 6            /* Time_mean of agent A-1                                                                    */
#define GMPE_EVAL_TIME_FAIRNESS 7        /* Time_mean_by_stddev of agent A-1                                                          */
#define GMPE_EVAL_STDDEV_PARAM 8         /* 1 / (Distance_variance[A-1] + 0.0001)                                                     */
#define GMPE_EVAL_TIME_STDDEV_PARAM 9    /* 1 / (Time_stddev[A-1] + 0.0001)                                                           */
#define GMPE_EVAL_TOTAL_DISTS 10         /* sum over agents of Dists_traveled                                                         */
#define GMPE_EVAL_TOTAL_TIME 11          /* sum over agents of ttg                                                                    */
#define GMPE_EVAL_CONFORMANCE 12         /* mean over agents of Conformance                                                           */
#define GMPE_EVAL_DELTA_SPACE 13         /* mean over agents of Delta_spacing                                                         */
#define GMPE_EVAL_SPACING_VIOLATIONS 14  /* mean over agents of Spacing_violations                                                     */
#define GMPE_EVAL_STEPS 15               /* episode length (0: not finished)                                                          */
typedef struct gmpe_episode_record_plan {
    int32_t num_envs, num_agents;   /* N >= 1, 1 <= A <= GMPE_MAX_AGENTS                                                            */
    int32_t t, num_steps;           /* step index 0 <= t < T = episode_length                                                      */
    int32_t n_actions;              /* row width of available_actions, 1 .. 4096                                                   */
    int32_t rnn_row;                /* R * H floats per agent of rnn_states, 1 .. 2^20 with rnn_states, else ignored               */
    const float* reward;            /* [N, A]       the step's outputs (gmpe_outputs of the engine)                                 */
    const uint8_t* done;            /* [N, A]                                                                                       */
    const float* info;              /* [N, A, GMPE_EVAL_INFO_WIDTH]                                                                 */
    uint8_t* live;                  /* [N]          state: 1 until the env's episode ends (the caller sets 1 at the reset)           */
    int32_t* steps;                 /* [N]          state: episode length once finished                                             */
    double* ret;                    /* [N, A]       state: sum of rewards                                                           */
    float* final_info;              /* [N, A, GMPE_EVAL_INFO_WIDTH] state: the info rows of the terminal step                        */
    float* masks;                   /* [N, A]       out                                                                             */
    float* available_actions;       /* [N, A, n_actions] out                                                                        */
    float* rnn_states;              /* [N, A, rnn_row] in place, or NULL                                                            */
} gmpe_episode_record_plan;
int gmpe_episode_record(int device, const gmpe_episode_record_plan* plan, void* stream);

/* gmpe_episode_record_series: gmpe_episode_record for R episodes per env played back to back across the engine's auto-resets (the render loop's
 * `for episode in range(render_episodes)`). There is no global step index: env n carries episode[n] in 0 .. R and t_in_ep[n]. One call per env step
 * on the same stream; for an env with episode[n] = e < R:
 *   ret[n, a] += double(reward[n, a]); t_in_ep[n] += 1; when every agent of env n is done or t_in_ep[n] == T (so T must be the engine's
 *   episode_length: an episode has to end where the engine resets): steps[e, n] = t_in_ep[n], ret_out[e, n] = ret[n], final_info[e, n] = info[n],
 *   then episode[n] = e + 1, t_in_ep[n] = 0, ret[n] = 0. The terminal step's reward belongs to the episode it ends.
 * An env with episode[n] == R is frozen. The outputs are episode-major: row e * N + n of the [R * N, ...] arrays is one episode, which is what
 * gmpe_episode_metrics (num_envs = R * N) and gmpe_episode_summary (num_rows = R * N) read. masks, available_actions and rnn_states are written
 * for every env by gmpe_episode_record's rules, so an env that just ended an episode acts next on the auto-reset observation with ones and zeroed
 * RNN rows. The caller zeroes episode, t_in_ep and ret at the reset. With R = 1 every state and output equals gmpe_episode_record's. */
typedef struct gmpe_episode_series_plan {
    int32_t num_envs, num_agents;   /* N >= 1, 1 <= A <= GMPE_MAX_AGENTS                                                            */
    int32_t num_steps;              /* T = the engine's episode_length >= 1                                                         */
    int32_t num_episodes;           /* R >= 1 episodes per env, R * N <= 2^31 - 1 (gmpe_episode_summary's row limit)                */
    int32_t n_actions;              /* row width of available_actions, 1 .. 4096                                                   */
    int32_t rnn_row;                /* R * H floats per agent of rnn_states, 1 .. 2^20 with rnn_states, else ignored               */
    const float* reward;            /* [N, A]       the step's outputs (gmpe_outputs of the engine)                                 */
    const uint8_t* done;            /* [N, A]                                                                                       */
    const float* info;              /* [N, A, GMPE_EVAL_INFO_WIDTH]                                                                 */
    int32_t* episode;               /* [N]          state: episodes this env has completed, 0 .. R                                  */
    int32_t* t_in_ep;               /* [N]          state: steps booked to the env's running episode                                */
    double* ret;                    /* [N, A]       state: the running episode's sum of rewards                                     */
    int32_t* steps;                 /* [R, N]       out: episode lengths                                                            */
    double* ret_out;                /* [R, N, A]    out: episode returns                                                            */
    float* final_info;              /* [R, N, A, GMPE_EVAL_INFO_WIDTH] out: the info rows of each episode's terminal step            */
    float* masks;                   /* [N, A]       out                                                                             */
    float* available_actions;       /* [N, A, n_actions] out                                                                        */
    float* rnn_states;              /* [N, A, rnn_row] in place, or NULL                                                            */
} gmpe_episode_series_plan;
int gmpe_episode_record_series(int device, const gmpe_episode_series_plan* plan, void* stream);

/* gmpe_episode_metrics: one f64 row of the GMPE_EVAL_* columns per env from its record, ttg_a = Time_req_to_goal with -1 -> T*dt
 * (base_runner.py:214-217; the reference never assigns the runner's dt: the world's dt is meant). Sums and means over agents follow NumPy's
 * pairwise order, so every column equals the reference's float64 NumPy on the same f32 info rows bit for bit. The same launch writes the
 * per-agent sums over episodes dists_traveled[A] (Dists_traveled) and time_taken[A] (ttg), the render loop's dists_trav_list / time_taken_list
 * (:680-686), as a fixed-order tree over the N envs: no atomics, bitwise reproducible. One launch. */
typedef struct gmpe_episode_metrics_plan {
    int32_t num_envs, num_agents, num_steps, reserved;  /* N, A, T as recorded; reserved 0                                          */
    double dt;                      /* > 0                                                                                          */
    double min_dist_thresh;         /* success threshold on Dist_to_goal                                                            */
    const int32_t* steps;           /* [N]                                                                                          */
    const double* ret;              /* [N, A]                                                                                       */
    const float* final_info;        /* [N, A, GMPE_EVAL_INFO_WIDTH]                                                                 */
    double* episodes;               /* [N, GMPE_EVAL_NUM_COLUMNS] out                                                               */
    double* dists_traveled;         /* [A] out, or NULL (then time_taken too)                                                       */
    double* time_taken;             /* [A] out, or NULL                                                                             */
} gmpe_episode_metrics_plan;
int gmpe_episode_metrics(int device, const gmpe_episode_metrics_plan* plan, void* stream);

/* gmpe_episode_summary: per column of an f64 [n, num_columns] row-major table, the row of GMPE_EVAL_STAT_* values. Order statistics are exact
 * (radix selection of the ranks on the f64 bit patterns) and then combined as NumPy 2.x does: p10 / p90 = np.percentile(x, q) with the default
 * linear method (index (n-1) * (q/100), its floor and floor + 1, _lerp with its t >= 0.5 branch), median = np.median (the middle element, or the
 * two middle ones added and halved). A NaN in a column makes its order statistics NaN, as in NumPy. Mean and population std (np.std) in f64 with a
 * fixed-order tree. Column `success_column` (or none when < 0) holds per-episode means over `success_agents` 0/1 values: its statistics are
 * those of the flattened [n, success_agents] 0/1 matrix, as the render loop's success_rates_arr (:784-789). One workgroup per column, one launch. */
#define GMPE_EVAL_STAT_MIN 0
#define GMPE_EVAL_STAT_P10 1
#define GMPE_EVAL_STAT_MEDIAN 2
#define GMPE_EVAL_STAT_P90 3
#define GMPE_EVAL_STAT_MAX 4
#define GMPE_EVAL_STAT_MEAN 5
#define GMPE_EVAL_STAT_STD 6
#define GMPE_EVAL_NUM_STATS 7
typedef struct gmpe_episode_summary_plan {
    int64_t num_rows;               /* n, 1 .. 2^31 - 1                                                                             */
    int32_t num_columns;            /* 1 .. 64                                                                                      */
    int32_t success_column;         /* -1 or a column index                                                                         */
    int32_t success_agents;         /* 1 .. GMPE_MAX_AGENTS when success_column >= 0                                                */
    int32_t reserved;               /* 0                                                                                            */
    const double* table;            /* [n, num_columns]                                                                             */
    double* out;                    /* [num_columns, GMPE_EVAL_NUM_STATS]                                                           */
} gmpe_episode_summary_plan;
int gmpe_episode_summary(int device, const gmpe_episode_summary_plan* plan, void* stream);

/* ---- run()'s log and eval intervals on device data (handle-less): Runner.process_infos + log_env (base_runner.py:194-302) and the bookkeeping of
 * GMPERunner.eval (graph_mpe_runner.py:445-516). No allocation, no workspace, no host synchronisation, every launch on `stream`.
 *
 * gmpe_env_infos: out[a, k] = np.mean of the N Python floats float(info[n, a, k]), n = 0 .. N-1, bit for bit: float64 NumPy's add.reduce takes
 * the values in consecutive chunks of GMPE_INFOS_CHUNK, starts from +0.0 and adds each chunk's pairwise_sum in order (a piece of more than
 * GMPE_INFOS_LEAF values splits at n2 = n/2 - (n/2) % 8; a smaller one is summed by eight accumulators, their tree, then the tail; fewer than 8
 * values sequentially), then divides by N. In column Time_req_to_goal a value of exactly -1 counts as (double)episode_length * dt
 * (base_runner.py:215-216). A NaN in a column gives that column NaN. */
#define GMPE_INFOS_CHUNK 8192            /* NumPy's reduce buffer, in elements                                                          */
#define GMPE_INFOS_LEAF 128              /* pairwise_sum's PW_BLOCKSIZE                                                                 */
typedef struct gmpe_env_infos_plan {
    int32_t num_envs;               /* N >= 1                                                                                       */
    int32_t num_agents;             /* 1 .. GMPE_MAX_AGENTS                                                                         */
    int32_t episode_length;         /* >= 1: all_args.episode_length                                                                */
    int32_t reserved;               /* 0                                                                                            */
    double dt;                      /* finite: the runner's dt                                                                      */
    const float* info;              /* [N, A, GMPE_INFO_KEYS]                                                                       */
    double* out;                    /* [A, GMPE_INFO_KEYS] out                                                                      */
} gmpe_env_infos_plan;
int gmpe_env_infos(int device, const gmpe_env_infos_plan* plan, void* stream);

/* gmpe_eval_step, once behind each env step of the eval episode, same stream:
 *   sums[n, a] = (first ? +0.0 : sums[n, a]) + double(reward[n, a]) — np.sum(np.array(eval_episode_rewards), axis=0): one add per step, in step order;
 *   masks[n, a, 0] = 0 where every agent of env n is done, else 1 (:500-505; per env, not per agent);
 *   rnn_states[n, :, :, :] = 0 where every agent of env n is done (:495-499); other rows are left as they are.
 * first = 1 stores instead of adding, so `sums` needs no memset. */
typedef struct gmpe_eval_step_plan {
    int32_t num_envs;               /* N >= 1                                                                                       */
    int32_t num_agents;             /* 1 .. GMPE_MAX_AGENTS                                                                         */
    int32_t rnn_row;                /* recurrent_N * hidden_size, 1 .. 2^20 with rnn_states, else 0                                 */
    int32_t first;                  /* 0 or 1                                                                                       */
    const float* reward;            /* [N, A]                                                                                       */
    const uint8_t* done;            /* [N, A]                                                                                       */
    double* sums;                   /* [N, A] state                                                                                 */
    float* masks;                   /* [N, A, 1] out                                                                                */
    float* rnn_states;              /* [N, A, rnn_row] in place; may be NULL                                                        */
} gmpe_eval_step_plan;
int gmpe_eval_step(int device, const gmpe_eval_step_plan* plan, void* stream);

/* gmpe_eval_mean: out[0] = np.mean of `count` contiguous float64 values, bit for bit, in gmpe_env_infos' order (log_env's mean of the [N, A] sums). */
typedef struct gmpe_eval_mean_plan {
    int64_t count;                  /* 1 .. 2^40                                                                                    */
    const double* values;           /* [count]                                                                                      */
    double* out;                    /* [1] out                                                                                      */
} gmpe_eval_mean_plan;
int gmpe_eval_mean(int device, const gmpe_eval_mean_plan* plan, void* stream);

/* PPO minibatches from a rollout (GraphReplayBuffer.feed_forward_generator / recurrent_generator, onpolicy/utils/graph_buffer.py:368-758): one minibatch's rows
 * of every field gathered from the [T+1, N, ...] arrays through a device permutation, as exact byte copies (16-byte vectors where row size and alignment allow)
 * or, for the table kinds, expanded from the f64 entity table with the arithmetic of gmpe_expand_node_obs / gmpe_expand_adj (bit-identical to the engine).
 * Output row r of a minibatch reads sample (t, n, a):
 *   GMPE_MB_FEED_FORWARD: j = perm[offset + r] over the [T, N, A] flattening: t = j / (N*A), n = (j / A) % N, a = j % A. Output rows: `rows`.
 *   GMPE_MB_RECURRENT:    the samples in [N, A, T] order (graph_buffer.py:15-16 _cast) cut into chunks of L; r = l * rows + k (np.stack(axis=1) then _flatten),
 *                         c = perm[offset + k], f = c*L + l: n = f / (A*T), a = (f / T) % A, t = f % T (a chunk may cross agent and env boundaries when
 *                         T % L != 0). Output rows: rows * L; GMPE_MB_CHUNK_HEAD fields: `rows`, from each chunk's first sample f = c*L.
 * Permutation entries outside [0, T*N*A) (feed-forward) or [0, T*N*A / L) (recurrent) are not read: their output rows are left unwritten.
 * Handle-less: `cfg` (NULL allowed without table kinds) supplies scenario, feature type and E / W for the table kinds. No allocation, no host synchronisation,
 * no atomics; one launch, two with table kinds, on `stream`: capturable in a hipGraph. Every argument the host can see is checked before any device call. */
#define GMPE_MB_FEED_FORWARD 0
#define GMPE_MB_RECURRENT 1
#define GMPE_MB_ROW 0          /* row of sample (t, n, a): src + t * slot_stride + (n*A + a) * row_bytes                                          */
#define GMPE_MB_ENV_ROW 1      /* row of env-step (t, n):  src + t * slot_stride + n * row_bytes (compact adj; share_obs = obs[t, n] with A*D floats)   */
#define GMPE_MB_CHUNK_HEAD 2   /* recurrent only: GMPE_MB_ROW addressing, one output row per chunk (rnn_states / rnn_states_critic)                */
#define GMPE_MB_TABLE_NODE 3   /* node rows of ego a at (t, n) from the entity table src + t * slot_stride + n * W * 8: row_bytes = E * F * 4          */
#define GMPE_MB_TABLE_ADJ 4    /* the E x E matrix of (t, n) from the entity table: row_bytes = E * E * 4                                          */
#define GMPE_MB_MAX_FIELDS 20
typedef struct gmpe_mb_field {
    int32_t kind;               /* GMPE_MB_ROW .. GMPE_MB_TABLE_ADJ                                                                         */
    int32_t row_bytes;          /* bytes of one OUTPUT row (a multiple of 4); source rows have the same size except for the table kinds     */
    int64_t slot_stride;        /* bytes between slot t and t + 1 of src (at least one slot: N*A rows, N rows, or N*W doubles)             */
    const void* src;            /* slot 0 of the source array, device memory (8-byte aligned for the table kinds)                          */
    void* dst;                  /* output rows, row_bytes apart, device memory                                                              */
} gmpe_mb_field;
typedef struct gmpe_minibatch_plan {
    int32_t mode;               /* GMPE_MB_FEED_FORWARD or GMPE_MB_RECURRENT                                                                */
    int32_t num_fields;         /* 1 .. GMPE_MB_MAX_FIELDS                                                                                  */
    int32_t T, N, A;            /* episode length, envs, agents of the arrays (T*N*A < 2^31); A = cfg->num_agents with table kinds           */
    int32_t L;                  /* data_chunk_length (recurrent), >= 1; ignored feed-forward                                                */
    const int64_t* perm;        /* device permutation: samples (feed-forward) or chunks (recurrent)                                         */
    int64_t perm_len;           /* its entries                                                                                              */
    int64_t offset;             /* first entry of this minibatch                                                                            */
    int64_t rows;               /* samples (feed-forward) or chunks (recurrent) of this minibatch: offset + rows <= perm_len                 */
    gmpe_mb_field fields[GMPE_MB_MAX_FIELDS];
} gmpe_minibatch_plan;
int gmpe_minibatch_gather(const gmpe_config* cfg, int device, const gmpe_minibatch_plan* plan, void* stream);

/* The edge list of a minibatch straight from the adjacency the rollout stores: what TransformerConvNet.process_adj (onpolicy/algorithms/utils/gnn_new.py:329-358)
 * makes of the adj_batch that gmpe_minibatch_gather would write, without that [rows, E, E] tensor. Graph r is output row r of gmpe_minibatch_gather: the same
 * (t, n, a) from the same mode, perm, offset, rows, L (the map above; recurrent: rows * L graphs, r = l * rows + k). perm == NULL is the identity, entry k = offset + k:
 * the edges of one rollout step are the feed-forward call with T = 1, rows = N * A and `src` at that slot.
 * Rule: (adj < max_edge_dist) & (adj > 0) on fp32 (`inclusive`: <=), edges in (graph, row i, col j) lexicographic order, node ids r*E + i and r*E + j,
 * edge_attr the adjacency value. Only the first `cap` edges are written; n_edges holds the true count (saturating at INT32_MAX) whatever `cap` is.
 * A graph whose permutation entry is out of range has zero edges and its source is not read (the gather leaves such rows unwritten; an edge list cannot).
 * Three launches on `stream` (per-graph count, scan of the per-workgroup totals in fixed chunks, ordered write): no atomics, no allocation, no host
 * synchronisation, capturable in a hipGraph, same input -> same bits. Count-only call: edge_index == NULL runs count + scan and leaves n_edges and the offsets
 * in the workspace; a following call on the same workspace and the same plan with `reuse_counts` runs the write alone (n_edges is then left as it is).
 * Every argument the host can see is checked before any device call. */
#define GMPE_MBE_ADJ 0          /* src f32 [T+1, N, A, E, E]: graph r reads ego a's copy                                                          */
#define GMPE_MBE_ADJ_COMPACT 1  /* src f32 [T+1, N, E, E]: graph r reads (t, n)                                                                      */
#define GMPE_MBE_TABLE 2        /* src f64 entity table [T+1, N, W]: entries rebuilt as GMPE_MB_TABLE_ADJ does (needs cfg; E, A must be the config's) */
typedef struct gmpe_mb_edges_plan {
    int32_t mode;               /* GMPE_MB_FEED_FORWARD or GMPE_MB_RECURRENT                                                                */
    int32_t source;             /* GMPE_MBE_*                                                                                               */
    int32_t T, N, A;            /* episode length, envs, agents of the source (T*N*A < 2^31)                                               */
    int32_t L;                  /* data_chunk_length (recurrent), >= 1; ignored feed-forward                                                */
    int32_t E;                  /* nodes per graph, 1 .. GMPE_MAX_ENTITIES                                                                  */
    int32_t inclusive;          /* 0: adj < max_edge_dist; 1: adj <= max_edge_dist                                                          */
    int32_t index64;            /* 0: edge_index int32 (graphs * E must fit); 1: int64                                                      */
    int32_t reuse_counts;       /* 1: the workspace holds the counts of a count-only call on this plan: write only (needs edge_index)      */
    float max_edge_dist;        /* not NaN                                                                                                  */
    int32_t reserved;           /* 0                                                                                                        */
    const int64_t* perm;        /* device permutation (samples feed-forward, chunks recurrent), or NULL: the identity                       */
    int64_t perm_len;           /* its entries (ignored with perm == NULL)                                                                  */
    int64_t offset;             /* first entry of this minibatch                                                                            */
    int64_t rows;               /* samples (feed-forward) or chunks (recurrent) of this minibatch; with a perm offset + rows <= perm_len     */
    const void* src;            /* slot 0 of the source, device memory (4-byte aligned; 8-byte for GMPE_MBE_TABLE)                          */
    int64_t slot_stride;        /* bytes between slot t and t + 1 of src (at least one slot)                                                */
    void* edge_index;           /* [2, cap] int32 / int64 (row 0 sources, row 1 destinations), or NULL: count only                          */
    float* edge_attr;           /* [cap] (needed with edge_index)                                                                           */
    int64_t cap;                /* >= 0                                                                                                     */
    int32_t* n_edges;           /* [1] device                                                                                               */
    void* workspace;            /* device scratch of gmpe_minibatch_edges_workspace_bytes(graphs) bytes, 8-byte aligned                     */
    size_t workspace_bytes;
} gmpe_mb_edges_plan;
/* bytes of workspace for `graphs` graphs (rows feed-forward, rows * L recurrent): the per-workgroup offsets (int64) followed by the per-graph counts (int32) */
int gmpe_minibatch_edges_workspace_bytes(int64_t graphs, size_t* bytes_out);
int gmpe_minibatch_edges(const gmpe_config* cfg, int device, const gmpe_mb_edges_plan* plan, void* stream);

/* What gmpe_create chose for this handle (recorded by bench.py next to every number). Environment variables override the heuristics —
 * GMPE_G / GMPE_BLOCK (step tile shape), GMPE_GROLL (rollout tile shape), GMPE_AP=0 (run-time-size instead of exact-size kernels),
 * GMPE_NT / GMPE_ROLLNT (nontemporal graph stores of step / rollout launches), GMPE_SPEC (wave specialisation), GMPE_SPLIT / GMPE_CHUNKS
 * / GMPE_RAMP / GMPE_AHEAD / GMPE_XSTEP (split big-E path, its chunk count, quarter + half first chunks, run-ahead bound, chained steps), GMPE_ROLL (gmpe_step_many as one rollout launch), GMPE_FUSE — none of them changes results
 * (tests/test_gpu_instantiations.py, tests/test_gpu_rollout_kernel.py). */
typedef struct gmpe_tuning {
    int32_t G;                  /* envs per workgroup (tile)                                               */
    int32_t block;              /* threads per workgroup: 64, 128 or 256                                   */
    int32_t nt;                 /* 1: nontemporal graph stores (launch output > Infinity Cache)            */
    int32_t spec;               /* 1: wave-specialised tiles                                               */
    int32_t split;              /* 1: big-E path — fused kernel writes the compact [N,E,E] matrix into the handle's scratch,
                                      k_adj_expand materialises the A ego copies                           */
    int32_t roll;               /* 1: gmpe_step_many runs the persistent rollout kernel                    */
    int32_t ap;                 /* exact-size instantiation (0: run-time sizes)                            */
    int32_t lds_bytes;          /* dynamic LDS per tile of the step kernels                                */
    int32_t diag_build;         /* 1: library built with -DGMPE_DIAG (ablations honoured): never for results */
    int32_t G_roll, block_roll; /* tile shape of the rollout kernel (its own register budget, hence its own residency)  */
    int32_t chunks, ahead;      /* split path: env chunks per step; how many chunks the fused kernel may run ahead of the expansion (0: unbounded) */
    int32_t xstep;              /* split path: gmpe_step_many chains the steps' chunk pipelines (no join between open-loop steps)          */
    int32_t chunks_x, ahead_x;  /* ... with this chunking / run-ahead bound                                                                */
    int32_t lds_bytes_roll;     /* dynamic LDS per tile of the rollout kernel (G_roll envs; + the pair-force buffer of fused navigation_graph rollouts)     */
} gmpe_tuning;
int gmpe_get_tuning(const gmpe_handle* h, gmpe_tuning* out);

/* Timing hooks used by bench.py: HIP events on the handle's launch stream around every step
 * kernel, so the dominant kernel's duration is measured live (not via torch's current stream). */
int gmpe_timing_enable(gmpe_handle* h, int32_t enable);          /* one event pair around EVERY launch (perturbs back-to-back launches by ~5 us each) */
int gmpe_timing_read(gmpe_handle* h, double* total_ms, int64_t* launches, int32_t reset_counters);
/* one event pair around a REGION of launches: mark(0) before the first, mark(1) after the last, both on
 * the launch stream; region_ms synchronises on the second event. */
int gmpe_timing_mark(gmpe_handle* h, int32_t which, void* stream);
int gmpe_timing_region_ms(gmpe_handle* h, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* GMPE_H */
