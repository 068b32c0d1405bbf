"""Bit-for-bit A/B of two builds of libgmpe.so over the three entry points that share gmpe_ppo_rows.h: gmpe_ppo_loss, gmpe_ppo_loss_popart and
gmpe_act_sample, over gmpe_compute_returns and the two sharded entry points, and over the nine entry points of the three layer kernels (gmpe_gru_*,
gmpe_mlp_*, gmpe_gnn_*) and the two wide forwards (gmpe_gnn_forward_wide, _wide_table), called through their C plans on fixed inputs. The GPU suites bound the losses and the layers against float64, so they would
not see a changed rounding or a changed order of the finish sums; this does.

    GMPE_LIB=/path/to/libgmpe_parent.so python tools/learner_ab_bits.py dump a.npz     # one process per build
    python tools/learner_ab_bits.py dump b.npz
    python tools/learner_ab_bits.py compare a.npz b.npz                                 # exit 1 unless every array is equal as integers

Inputs: the generators of tests/ppo_loss_lib.py ("edges": +-30 logits, stop rows, rows with nothing available), tests/popart_lib.py (a layer and
features for the values) and tests/act_lib.py ("wide", with empty rows). rows in 1, 255, 257, 600 (one lane; a tile less one; one and two tiles and a
bit) x K in 1, 2, 5, 25, 64 (tile_copy's K == 1 branch; even: S = K + 1; odd: S = K; the 64-bit mask and the raised LDS limit) x base pointers 16-byte
aligned / offset by one element (the 4-byte path) x actions float32 / int64 x available_actions given / absent x all flags on / off; PopArt with
H in 1, 7, 64, 1024 laid over (rows, K) as a Latin square, so every (rows, H) and every (K, H) occurs; act with the availability from an array, from
dones_prev and from neither x deterministic 0 / 1 x draw_dev given (the counter after the call is kept) / absent. Every call is tiny.
Kept per call: the seven float64 scalars, every gradient, action_log_probs, imp_weights, values, the updated normaliser state and the rescaled layer;
action_idx, both action arrays, the log-probs.
returns/: gmpe_compute_returns with normalised advantages on tests/returns_lib.py's branch_inputs (T in 8, 9, 17, 65 at 65 lanes; the recurrence in its
eight branches and the advantages alone with and without a denormaliser) and on every tests/learner_shards_lib.py RETURNS_CASES x both paths; the same
inputs through gmpe_compute_returns_shard LOCAL then APPLY at world 1, and the cases at their own split with `all` stacked from the shards' `local`.
shard/: gmpe_ppo_loss_shard LOCAL then APPLY for rows in 1, 257, 600 x K in 1, 5, 64 x all flags on / off at world 1, and 1030 rows split 1 + 256 + 773.
Kept: returns, value_preds, raw and normalised advantages, `local`; the loss call's outputs as above with `local`.
layers/: every case once through its forward-only plan and once through its training plan (forward with the workspace, then backward), the workspace
of the size its *_workspace_bytes entry gives. gru/: tests/gru_lib.py's CASES x PATTERNS, and (1, 8257) (259 tiles on 256 workgroups) and (17, 241)
(ragged and empty parts, tests/layer_scale_lib.py's GRU_SIZE_SHAPES) with random masks. mlp/: tests/mlp_lib.py's CASES and layer_scale_lib's 545-,
8257- and 32801-row cases, at mlp_lib's seed 0. gnn/: tests/gnn_lib.py's CASES, and 5005 graphs of E = 6 (the 65 of the actor's case repeated: every
workgroup of backward owns several tiles, the finish adds 256 partial rows) with a dense adjacency and with one matrix shared by five rows.
Kept: features (and hxs_out) of both plans, every input gradient, every parameter gradient, the workspace size.
gnnwide/: gmpe_gnn_forward_wide on tests/gnn_lib.py's inputs at E = 65 (W = 2), 87 | 88 (W = 2 | 1 at the shipped sizes) and 128 with the four
aggregates and the largest configuration; 1, 2, 3 and 513 graphs of E = 65 (an idle pair; a workgroup with two tiles); one matrix serving three rows;
gmpe_gnn_forward_wide_table on the tables of a stepped navigation_graph engine at E = 65 and 128 (tests/test_gpu_gnn_wide.py's), actor and critic, with
an int32 index, an int64 index and a table_share. Kept: features. The GPU suite bounds nodes above 64 against float64 only.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS, KS, HS = (1, 255, 257, 600), (1, 2, 5, 25, 64), (1, 7, 64, 1024)
COLS = ("value_preds", "returns", "active_masks", "old_action_log_probs", "adv_targ")
HYPER = dict(clip_param=0.2, huber_delta=10.0, entropy_coef=0.01, beta=0.99999, epsilon=1e-5)


def dump(path):
    import torch
    import gmpe  # noqa: F401
    from gmpe import _lib
    import act_lib
    import popart_lib
    import ppo_loss_lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    kept, keep = {}, []

    def put(a, off, dtype=None):
        """`a` on the device, its base 16-byte aligned (off 0) or one element past that (off 1)."""
        src = torch.from_numpy(np.array(a, dtype=dtype, order="C"))      # a copy: the cases are read-only arrays
        buf = torch.zeros(src.numel() + 1, dtype=src.dtype, device=dev)
        t = buf[off:off + src.numel()].view(src.shape)
        t.copy_(src)
        assert t.data_ptr() % 16 == (off * src.element_size()) % 16
        keep.append(buf)
        return t

    def blank(shape, off, dtype=np.float32):
        return put(np.zeros(shape, dtype), off)

    def ptr(t):
        return None if t is None else t.data_ptr()

    def save(tag, **arrays):
        torch.cuda.synchronize()
        for k, t in arrays.items():
            kept["%s/%s" % (tag, k)] = t.cpu().numpy()
        del keep[:]

    def minibatch(plan, inp, K, off, act64, given, flags):
        B = inp["logits"].shape[0]
        plan.rows, plan.n_actions, plan.flags, plan.actions_int64 = B, K, flags, int(act64)
        for k, v in HYPER.items():
            setattr(plan, k, v)
        plan.logits = ptr(put(inp["logits"], off))
        plan.actions = ptr(put(inp["actions"], off, np.int64 if act64 else np.float32))
        plan.available_actions = ptr(put(inp["available_actions"], off)) if given else None
        for k in COLS:
            setattr(plan, k, ptr(put(inp[k], off)))
        out = dict(out=blank(_lib.PPO_NUM_OUT, 0, np.float64), grad_logits=blank((B, K), off), action_log_probs=blank((B, 1), off),
                   imp_weights=blank((B, 1), off))
        for k, t in out.items():
            setattr(plan, k, ptr(t))
        return out

    variants = list(itertools.product((0, 1), (False, True), (True, False), (True, False)))      # off, int64 actions, avail given, flags on
    for ri, B in enumerate(ROWS):
        for ki, K in enumerate(KS):
            inp = ppo_loss_lib.family("edges", B, K, masks="mixed")
            for off, act64, given, on in variants:
                tag = "B%d_K%d_off%d_i64%d_av%d_fl%d" % (B, K, off, act64, given, on)
                # ---- gmpe_ppo_loss
                plan = _lib.GmpePpoLossPlan()
                out = minibatch(plan, inp, K, off, act64, given, 31 if on else 0)
                plan.values = ptr(put(inp["values"], off))
                out["grad_values"] = blank((B, 1), off)
                plan.grad_values = ptr(out["grad_values"])
                if on:
                    for k, v in (("running_mean", 0.3), ("running_mean_sq", 1.7), ("debiasing_term", 0.5)):
                        out[k] = put(np.full(1, v, np.float32), off)
                        setattr(plan, k, ptr(out[k]))
                n = C.c_size_t()
                _lib.check(lib.gmpe_ppo_loss_workspace_bytes(B, C.byref(n)), "gmpe_ppo_loss_workspace_bytes")
                ws = torch.zeros(n.value, dtype=torch.uint8, device=dev)
                plan.workspace, plan.workspace_bytes = ws.data_ptr(), n.value
                _lib.check(lib.gmpe_ppo_loss(dev.index, C.byref(plan), stream), "gmpe_ppo_loss")
                save("loss/" + tag, **out)
                # ---- gmpe_ppo_loss_popart
                H = HS[(ri + ki) % len(HS)]
                st = popart_lib.fresh_popart(H)
                st.update(stddev=np.full(1, 1.5, np.float32), mean=np.full(1, 0.25, np.float32), mean_sq=np.full(1, 2.0, np.float32),
                          debiasing_term=np.full((), 0.5, np.float32))
                plan = _lib.GmpePopartLossPlan()
                out = minibatch(plan, inp, K, off, act64, given, 15 if on else 0)
                plan.hidden = H
                plan.critic_features = ptr(put(popart_lib.features(inp["values"], st, H), off))
                for k in popart_lib.STATE:
                    out[k] = put(st[k].reshape(-1) if k != "weight" else st[k], off)
                    setattr(plan, k, ptr(out[k]))
                aliased = bool(off)                                          # the rescaled layer into new arrays, or over the old one
                for k in ("weight", "bias", "stddev"):
                    if not aliased:
                        out[k + "_out"] = blank(out[k].shape, off)
                    setattr(plan, k + "_out", ptr(out[k] if aliased else out[k + "_out"]))
                for k, shape in (("values_out", (B, 1)), ("grad_features", (B, H)), ("grad_weight", (1, H)), ("grad_bias", (1,))):
                    out[k] = blank(shape, off)
                    setattr(plan, k, ptr(out[k]))
                _lib.check(lib.gmpe_ppo_loss_popart_workspace_bytes(B, H, C.byref(n)), "gmpe_ppo_loss_popart_workspace_bytes")
                ws = torch.zeros(n.value, dtype=torch.uint8, device=dev)
                plan.workspace, plan.workspace_bytes = ws.data_ptr(), n.value
                _lib.check(lib.gmpe_ppo_loss_popart(dev.index, C.byref(plan), stream), "gmpe_ppo_loss_popart")
                save("popart_H%d/%s" % (H, tag), **out)
            # ---- gmpe_act_sample
            logits, av = act_lib.family("wide", B, K, avail="empty")
            dones = (np.random.RandomState(B * 131 + K).rand(B) < 0.3).astype(np.uint8)
            for off, source, det, counter in itertools.product((0, 1), ("array", "dones", "none"), (0, 1), (False, True)):
                plan = _lib.GmpeActPlan()
                plan.rows, plan.n_actions, plan.num_agents, plan.stop_action, plan.deterministic = B, K, 3, K // 2, det
                plan.env_id_base, plan.seed, plan.draw, plan.draw_inc = 1000, act_lib.SEED, act_lib.DRAW, 5
                plan.logits = ptr(put(logits, off))
                plan.available_actions = ptr(put(av, off)) if source == "array" else None
                plan.dones_prev = ptr(put(dones, off)) if source == "dones" else None
                out = dict(action_idx=blank(B, off, np.int32), log_probs=blank((B, 1), off), actions_f32=blank((B, 1), off),
                           actions_i64=blank((B, 1), 0, np.int64))
                if counter:
                    out["draw_dev"] = put(np.full(1, 7, np.int64), 0)
                    plan.draw_dev = ptr(out["draw_dev"])
                plan.action_idx, plan.log_probs = ptr(out["action_idx"]), ptr(out["log_probs"])
                plan.actions_f32, plan.actions_i64 = ptr(out["actions_f32"]), ptr(out["actions_i64"])
                _lib.check(lib.gmpe_act_sample(dev.index, C.byref(plan), stream), "gmpe_act_sample")
                save("act/B%d_K%d_off%d_%s_det%d_ctr%d" % (B, K, off, source, det, counter), **out)
    # ---- gmpe_compute_returns and gmpe_compute_returns_shard
    import learner_shards_lib as LS
    import returns_lib

    def returns_plan(d, flags, denorm):
        """d: float32 arrays [T(+1), lanes, 1] -> (plan, the arrays it writes)"""
        T, L = d["value_preds"].shape[0] - 1, d["value_preds"].shape[1]
        plan = _lib.GmpeReturnsPlan()
        plan.num_steps, plan.flags, plan.lanes, plan.stride, plan.gamma, plan.gae_lambda = T, flags, L, L, 0.99, 0.95
        out = dict(value_preds=put(d["value_preds"], 0), returns=put(d["returns"], 0), advantages=blank((T, L, 1), 0), normalized=blank((T, L, 1), 0))
        for k, t in out.items():
            setattr(plan, k, ptr(t))
        for k in ("rewards", "masks", "bad_masks", "next_value", "active_masks"):
            if k in d and not (flags & _lib.RETURNS_ADVANTAGES_ONLY and k != "active_masks"):
                setattr(plan, k, ptr(put(d[k], 0)))
        if denorm:
            plan.denorm_mean, plan.denorm_std = (ptr(put(np.full(1, v, np.float32), 0)) for v in returns_lib.DENORM)
        n = C.c_size_t()
        _lib.check(lib.gmpe_returns_workspace_bytes(L, C.byref(n)), "gmpe_returns_workspace_bytes")
        ws = torch.zeros(n.value, dtype=torch.uint8, device=dev)
        keep.append(ws)
        plan.workspace, plan.workspace_bytes = ws.data_ptr(), n.value
        return plan, out

    def shard_call(entry, sp, phase, world, local, all_stats):
        sp.phase, sp.world, sp.local, sp.all = phase, world, ptr(local), ptr(all_stats)
        _lib.check(getattr(lib, entry)(dev.index, C.byref(sp), stream), entry)

    def two_phase(entry, Shard, k, plans):
        """LOCAL on every shard's plan, `all` stacked from their `local`, APPLY on every shard -> the [world, k] tensor"""
        sps, locs = [], []
        for plan in plans:
            sp = Shard()
            sp.base = plan
            locs.append(torch.zeros(k, dtype=torch.float64, device=dev))
            shard_call(entry, sp, _lib.SHARD_LOCAL, 1, locs[-1], None)
            sps.append(sp)
        all_stats = torch.stack(locs).contiguous()
        for sp in sps:
            shard_call(entry, sp, _lib.SHARD_APPLY, len(plans), None, all_stats)
        return all_stats

    def returns_group(tag, d, flags, denorm, split):
        plan, out = returns_plan(d, flags, denorm)
        _lib.check(lib.gmpe_compute_returns(dev.index, C.byref(plan), stream), "gmpe_compute_returns")
        save("returns/%s/plain" % tag, **out)
        for name, bounds in (("world1", [(0, d["value_preds"].shape[1])]),) + ((("split", LS.bounds(split)),) if split else ()):
            made = [returns_plan({k: np.ascontiguousarray(v[:, lo:hi] if k != "next_value" else v[lo:hi]) for k, v in d.items()}, flags, denorm)
                    for lo, hi in bounds]
            all_stats = two_phase("gmpe_compute_returns_shard", _lib.GmpeReturnsShardPlan, _lib.RETURNS_SHARD_STATS, [m[0] for m in made])
            outs = {"%s_s%d" % (k, i): t for i, m in enumerate(made) for k, t in m[1].items()}
            save("returns/%s/%s" % (tag, name), local=all_stats, **outs)

    for T in (8, 9, 17, 65):
        d = returns_lib.branch_inputs(T)
        for gae, proper, dn in itertools.product((0, 1), repeat=3):
            returns_group("branch_T%d_gae%d_proper%d_dn%d" % (T, gae, proper, dn), d, gae * _lib.RETURNS_GAE | proper * _lib.RETURNS_PROPER_TIME_LIMITS, dn, None)
        for dn in (0, 1):
            returns_group("branch_T%d_only_dn%d" % (T, dn), d, _lib.RETURNS_ADVANTAGES_ONLY, dn, None)
    for name in LS.RETURNS_CASES:
        adv, am, split = LS.returns_case(name)
        for which in LS.PATHS:
            d = dict(returns_lib.prescribed_inputs(adv, which), active_masks=am.reshape(am.shape + (1,)))
            returns_group("%s_%s" % (name, which), d, _lib.RETURNS_ADVANTAGES_ONLY if which == "advantages" else 0, 0, split)

    # ---- gmpe_ppo_loss_shard
    def loss_plan(inp, K, on):
        B = inp["logits"].shape[0]
        plan = _lib.GmpePpoLossPlan()
        out = minibatch(plan, inp, K, 0, False, True, 31 if on else 0)
        plan.values = ptr(put(inp["values"], 0))
        out["grad_values"] = blank((B, 1), 0)
        plan.grad_values = ptr(out["grad_values"])
        if on:
            for k, v in (("running_mean", 0.3), ("running_mean_sq", 1.7), ("debiasing_term", 0.5)):
                out[k] = put(np.full(1, v, np.float32), 0)
                setattr(plan, k, ptr(out[k]))
        n = C.c_size_t()
        _lib.check(lib.gmpe_ppo_loss_workspace_bytes(B, C.byref(n)), "gmpe_ppo_loss_workspace_bytes")
        ws = torch.zeros(n.value, dtype=torch.uint8, device=dev)
        keep.append(ws)
        plan.workspace, plan.workspace_bytes = ws.data_ptr(), n.value
        return plan, out

    for B, split in [(B, (B,)) for B in (1, 257, 600)] + [(LS.ROWS, LS.LOSS_SPLITS[1])]:
        for K, on in itertools.product((1, 5, 64), (True, False)):
            inp = ppo_loss_lib.family("edges", B, K, masks="mixed")
            made = [loss_plan(LS.rows_of(inp, lo, hi), K, on) for lo, hi in LS.bounds(split)]
            all_stats = two_phase("gmpe_ppo_loss_shard", _lib.GmpePpoLossShardPlan, _lib.PPO_SHARD_STATS, [m[0] for m in made])
            outs = {"%s_s%d" % (k, i): t for i, m in enumerate(made) for k, t in m[1].items()}
            save("shard/B%d_K%d_fl%d_%s" % (B, K, on, "+".join(str(x) for x in split)), local=all_stats, **outs)
    # ---- the three layer kernels, each through its three entry points
    import gnn_lib
    import gru_lib
    import layer_scale_lib
    import mlp_lib
    from gmpe import gnn, gru, mlp

    def on_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def zeros(shape):
        return torch.zeros(tuple(shape), dtype=torch.float32, device=dev)

    def with_workspace(plan, ws):
        if ws is not None:
            plan.workspace, plan.workspace_bytes = ws.data_ptr(), ws.numel()
        return plan

    def layer(tag, name, nbytes, forward_plan, backward_plan):
        """forward_plan(workspace or None) -> (plan, its outputs), backward_plan(workspace) -> (plan, its gradients)"""
        plan, out = forward_plan(None)
        _lib.check(getattr(lib, name + "_forward")(dev.index, C.byref(plan), stream), name + "_forward")
        save("layers/%s/eval" % tag, **out)
        ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        plan, out = forward_plan(ws)
        _lib.check(getattr(lib, name + "_forward")(dev.index, C.byref(plan), stream), name + "_forward")
        plan, grads = backward_plan(ws)
        _lib.check(getattr(lib, name + "_backward")(dev.index, C.byref(plan), stream), name + "_backward")
        save("layers/%s/train" % tag, workspace_bytes=torch.tensor([nbytes.value]), **out, **grads)

    def gru_case(L, Nb, pattern):
        P, I, H = gru_lib.params(), gru_lib.inputs(L, Nb), gru_lib.H
        ps = [on_dev(P[k]) for k in gru_lib.PARAMS]
        x, hxs, gf, gh, m = (on_dev(a) for a in (I["x"], I["hxs"], I["gf"], I["gh"], gru_lib.masks(L, Nb, pattern)))
        n = C.c_size_t()
        _lib.check(lib.gmpe_gru_workspace_bytes(L, Nb, H, 1, C.byref(n)), "gmpe_gru_workspace_bytes")

        def forward_plan(ws):
            out = dict(features=zeros((L * Nb, H)), hxs_out=zeros((Nb, 1, H)))
            return gru._plan(L, Nb, gru_lib.D, H, gru_lib.EPS, x, hxs, m, ps, out["features"], out["hxs_out"], ws), out

        def backward_plan(ws):
            grads = {k: torch.zeros_like(t) for k, t in zip(gru_lib.GRADS, [x, hxs] + ps)}
            plan = gru._plan(L, Nb, gru_lib.D, H, gru_lib.EPS, x, hxs, m, ps, None, None, ws)
            plan.grad_features, plan.grad_hxs_out = ptr(gf), ptr(gh)
            for k, t in grads.items():
                setattr(plan, k, ptr(t))
            return plan, grads
        layer("gru/" + gru_lib.key(L, Nb, pattern), "gmpe_gru", n, forward_plan, backward_plan)

    def mlp_case(case):
        rows, dims, layer_n, act, fnorm = case
        P, I = mlp_lib.params(case), mlp_lib.inputs(case)
        ps = [on_dev(P[k]) for k in mlp_lib.param_names(case)]
        parts, gf = [on_dev(a) for a in mlp_lib.split(I["x"], dims)], on_dev(I["gf"])
        meta = (layer_n, mlp._ACTIVATIONS[act], fnorm, mlp_lib.EPS, (mlp_lib.EPS,) * (layer_n + 1))
        n = C.c_size_t()
        _lib.check(lib.gmpe_mlp_workspace_bytes(rows, sum(dims), mlp_lib.H, layer_n, 1, C.byref(n)), "gmpe_mlp_workspace_bytes")

        def forward_plan(ws):
            out = dict(features=zeros((rows, mlp_lib.H)))
            plan = with_workspace(mlp._plan(rows, dims, meta, parts, ps), ws)
            plan.features = ptr(out["features"])
            return plan, out

        def backward_plan(ws):
            grads = [torch.zeros_like(t) for t in parts + ps]
            plan = with_workspace(mlp._plan(rows, dims, meta, parts, ps), ws)
            plan.grad_features = ptr(gf)
            mlp._grads_into(plan, meta, grads[:len(parts)], grads[len(parts):])
            return plan, dict(zip(mlp_lib.out_names(case)[1:], grads))
        layer("mlp/" + mlp_lib.key(case), "gmpe_mlp", n, forward_plan, backward_plan)

    def gnn_case(tag, key, x, adj, ids, gf):
        names, ps, meta = gnn._base_params(gnn_lib.build(gnn_lib.CONFIGS[key]).to(dev))
        ps = [t.detach().contiguous() for t in ps]
        x, adj, ids, gf = x.to(dev).contiguous(), adj.to(dev).contiguous(), ids.to(device=dev, dtype=torch.int32), gf.to(dev).contiguous()
        (rows, E, F), (nemb, esz) = x.shape, ps[0].shape
        shape = (rows, E, F, rows // adj.shape[0], nemb, esz)
        n = C.c_size_t()
        _lib.check(lib.gmpe_gnn_workspace_bytes(C.byref(gnn._shape_plan(rows, E, F, shape[3], meta[0], meta[1], meta[2], nemb, esz)), 1, C.byref(n)),
                   "gmpe_gnn_workspace_bytes")

        def forward_plan(ws):
            out = dict(features=zeros((rows, gnn_lib.C)))
            plan = with_workspace(gnn._plan(shape, meta, x, adj, ids, ps), ws)
            plan.features = ptr(out["features"])
            return plan, out

        def backward_plan(ws):
            grads = [torch.zeros_like(t) for t in ps]
            plan = with_workspace(gnn._plan(shape, meta, x, adj, ids, ps), ws)
            plan.grad_features = ptr(gf)
            gnn._fill(plan, meta, meta[5], meta[2], meta[1], grads, "grad_")
            return plan, {"grad_" + k: t for k, t in zip(names, grads)}
        layer("gnn/" + tag, "gmpe_gnn", n, forward_plan, backward_plan)

    for (L, Nb), pattern in list(itertools.product(gru_lib.CASES, gru_lib.PATTERNS)) + [((1, 8257), "random"), ((17, 241), "random")]:
        gru_case(L, Nb, pattern)
    for case in mlp_lib.CASES + tuple(c for c in layer_scale_lib.MLP_CASES if c[0] in (545, 8257, 32801)):
        mlp_case(case)
    for case in gnn_lib.CASES:
        gnn_case(gnn_lib.case_id(case), case[2], *gnn_lib.inputs(*case)[:4])
    many, share = 5005, 5
    X, A, I, W = (t.repeat((many // 65,) + (1,) * (t.dim() - 1)) for t in gnn_lib.inputs(65, 6, gnn_lib.ACTOR)[:4])
    gnn_case("%dx6_dense" % many, gnn_lib.ACTOR, X, A, I, W)
    gnn_case("%dx6_shared%d" % (many, share), gnn_lib.ACTOR, X, A[:many // share], I, W)

    # ---- the forward at 65 .. 128 nodes, through gmpe_gnn_forward_wide and gmpe_gnn_forward_wide_table
    def wide_params(key):
        names, ps, meta = gnn._base_params(gnn_lib.build(gnn_lib.CONFIGS[key]).to(dev))
        return [t.detach().contiguous() for t in ps], meta

    def wide_case(tag, key, x, adj, ids):
        ps, meta = wide_params(key)
        x, adj, ids = x.to(dev).contiguous(), adj.to(dev).contiguous(), ids.to(device=dev, dtype=torch.int32)
        (rows, E, F), (nemb, esz) = x.shape, ps[0].shape
        out = zeros((rows, gnn_lib.C))
        plan = gnn._plan((rows, E, F, rows // adj.shape[0], nemb, esz), meta, x, adj, ids, ps)
        plan.features = ptr(out)
        _lib.check(lib.gmpe_gnn_forward_wide(dev.index, C.byref(plan), stream), "gmpe_gnn_forward_wide")
        save("gnnwide/rows/" + tag, features=out)

    def wide_table_case(tag, key, cfg, table, index, share, ids):
        ps, meta = wide_params(key)
        ids = ids.to(device=dev, dtype=torch.int32)
        rows, E, F, (nemb, esz) = ids.shape[0], cfg.num_entities, cfg.node_feats, ps[0].shape
        out = zeros((rows, gnn_lib.C))
        tp = gnn._table_plan((rows, E, F, 1, nemb, esz), meta, cfg, share, table, index, ids, ps)
        tp.base.features = ptr(out)
        _lib.check(lib.gmpe_gnn_forward_wide_table(dev.index, C.byref(tp), stream), "gmpe_gnn_forward_wide_table")
        save("gnnwide/table/" + tag, features=out)

    largest = gnn_lib.cfg_key(gnn_lib._RANDOM[-1])
    for n, E, key in ((5, 65, gnn_lib.ACTOR), (4, 87, gnn_lib.ACTOR), (4, 88, gnn_lib.ACTOR), (9, 128, gnn_lib.ACTOR), (9, 128, gnn_lib.CRITIC),
                      (9, 128, gnn_lib.ACTOR_MAX), (9, 128, gnn_lib.ACTOR_ADD), (3, 128, largest)):
        wide_case("%dx%d_%s" % (n, E, key), key, *gnn_lib.inputs(n, E, key)[:3])
    x, adj, ids = gnn_lib.inputs(9, 65, gnn_lib.ACTOR)[:3]
    for rows in (1, 2, 3):                              # one pair idle; a full tile; a second tile with an idle pair
        wide_case("%dx65" % rows, gnn_lib.ACTOR, x[:rows], adj[:rows], ids[:rows])
    wide_case("513x65", gnn_lib.ACTOR, x.repeat(57, 1, 1), adj.repeat(57, 1, 1), ids.repeat(57))      # 257 tiles on 256 workgroups
    envs, S = 2, 3
    wide_case("compact_%dx%dx66" % (envs, S), gnn_lib.ACTOR, gnn_lib.inputs(envs * S, 66, gnn_lib.ACTOR)[0], gnn_lib.inputs(envs, 66, gnn_lib.ACTOR)[1],
              torch.arange(S).repeat(envs))
    from gmpe.engine import GmpeEngine
    for tag, kw in (("nav65", dict(num_agents=30, num_obstacles=5, world_size=6.0, seed=96)), ("nav128", dict(num_agents=64, world_size=12.0, seed=97))):
        cfg = gmpe.make_config(scenario_name="navigation_graph", num_envs=2, episode_length=4, graph_feat_type="global", **kw)
        N, A = cfg.num_envs, cfg.num_agents
        eng = GmpeEngine(cfg, node_form="both", adj_compact=True)
        eng.reset()
        rng = np.random.RandomState(7)
        tabs = [eng.step(torch.as_tensor(rng.randint(0, cfg.n_actions, (N, A)).astype(np.int32))).entity_table.clone() for _ in range(6)]
        eng.check_errors()
        tabs = torch.stack(tabs).contiguous()            # [6, N, W]: past the time limit, so every env has reset
        g = torch.Generator().manual_seed(cfg.num_entities)
        index, ego = torch.randint(0, 6 * N, (11,), generator=g), torch.randint(0, A, (11,), generator=g)
        for key in (gnn_lib.ACTOR, gnn_lib.CRITIC):
            wide_table_case("%s_%s_index32" % (tag, key), key, cfg, tabs, index.to(device=dev, dtype=torch.int32), 1, ego)
            wide_table_case("%s_%s_index64" % (tag, key), key, cfg, tabs, index.to(dev), 1, ego)
            wide_table_case("%s_%s_share" % (tag, key), key, cfg, tabs[-1].contiguous(), None, A, torch.arange(A).repeat(N))
    np.savez(path, **kept)
    print("dump: %d arrays, %d elements (%d non-zero) from %s -> %s" % (len(kept), sum(a.size for a in kept.values()),
                                                                       sum(int(np.count_nonzero(a)) for a in kept.values()), _lib.LIB_PATH, path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = sorted(set(a.files) | set(b.files))
    differing = elements = 0
    for k in names:
        if k not in a.files or k not in b.files:
            print("only in one dump: %s" % k)
            differing += 1
            continue
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape:
            print("%s: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape))
            differing += 1
            continue
        bits = np.dtype("u%d" % x.dtype.itemsize)
        d = int((x.reshape(-1).view(bits) != y.reshape(-1).view(bits)).sum())
        elements += x.size
        if d:
            print("%s: %d of %d elements differ" % (k, d, x.size))
            differing += d
    per = {p: sum(1 for k in names if k.startswith(p)) for p in ("loss/", "popart_", "act/", "returns/", "shard/", "layers/", "gnnwide/")}
    print("compare: %d arrays (%s), %d elements, %d differing" % (len(names), ", ".join("%s %d" % (p.rstrip("/_"), n) for p, n in per.items()), elements,
                                                                 differing))
    return 1 if differing or not names else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
