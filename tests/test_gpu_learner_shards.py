"""The learner's batch statistics over several shards (include/gmpe.h gmpe_compute_returns_shard, gmpe_ppo_loss_shard) on one device, through the
two-step API: begin on every shard, torch.stack of the handles' .local, finish on every shard.

Returns: per shard, returns / side effects / raw advantages are the unsharded call's bits on the concatenated lanes; the normalised arrays of all shards
are fdiv(fsub(raw, m), d) for exactly one (m, d) of returns_lib.candidate_pairs over the concatenated data — the pair the float64 emulation of the
merge order (tests/learner_shards_lib.py: kernel order per shard, then Chan's merge as a left fold) ends at on the host.

PPO loss: the float64 restatement of tests/ppo_loss_lib.py over the CONCATENATED minibatch with the established bound C_DEV = 160 units of
U * (1 + |x|) (tests/test_gpu_ppo_loss.py's _check, unchanged): concatenated rows and gradients, the SUM of the shards' scalar rows, the ValueNorm
state; the DENOM columns exactly; the state bit-identical across shards.

world = 1 is the existing call bit for bit in both. The +-100 cases (shards whose means are near +100 and -100) are the ones an implementation that
exchanges nothing cannot pass."""
import types

import numpy as np
import pytest

import gmpe
import learner_shards_lib as LS
import ppo_loss_lib as P
import returns_lib as R
from gmpe import _lib

pytestmark = pytest.mark.gpu
OUT_KEYS = ("returns", "value_preds", "advantages", "normalized")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(x):
    import torch
    return torch.as_tensor(np.array(x), device="cuda")                  # a copy: the cases are read-only arrays


# ------------------------------------------------------------------------------------------------ returns
def _returns_arrays(name, path):
    """-> (arrays [T(+1), lanes, 1] (next_value [lanes, 1]), keywords of compute_returns, raw advantages expected [T, lanes], active_masks
    [T + 1, lanes], split, ascending: whether the statistics run over t ascending (k_advantages) or descending (k_returns))"""
    if name == "branch":
        T, L = LS.BRANCH_T, sum(LS.BRANCH_SPLIT)
        d = R.branch_inputs(T, L)
        d.pop("bad_masks")
        eadv = R.branch_expectations(dict(d, bad_masks=None), True, False, R.DENORM)[2]
        return d, dict(gamma=0.99, gae_lambda=0.95, use_gae=True, denorm=R.DENORM), R._rows(eadv), R._rows(d["active_masks"]), LS.BRANCH_SPLIT, False
    a, am, split = LS.returns_case(name)
    T, L = a.shape
    d = dict(R.prescribed_inputs(a, path), active_masks=am.reshape(T + 1, L, 1))
    kw = dict(advantages_only=True) if path == "advantages" else dict(gamma=0.99, gae_lambda=0.95, use_gae=False)
    return d, kw, a, am, split, path == "advantages"


def _lanes(d, lo, hi):
    return {k: (v[lo:hi] if k == "next_value" else v[:, lo:hi]) for k, v in d.items()}


def _kwargs(d, kw):
    import torch
    T, L = d["value_preds"].shape[0] - 1, d["value_preds"].shape[1]
    out = dict(rewards=None, masks=None)
    out.update({k: _dev(v) for k, v in d.items()})
    out.update(kw)
    if "denorm" in kw:
        out["denorm"] = tuple(torch.tensor([x], device="cuda") for x in kw["denorm"])
    out["advantages"], out["normalized"] = (torch.full((T, L, 1), -7.0, device="cuda") for _ in range(2))
    return out


def _read(k):
    return {n: k[n].cpu().numpy().reshape(k[n].shape[0], -1) for n in OUT_KEYS}


def _whole(d, kw):
    import torch
    k = _kwargs(d, kw)
    gmpe.engine.compute_returns(**k)
    torch.cuda.synchronize()
    return _read(k)


def _sharded(d, kw, split):
    """-> ({name: the shards' arrays side by side}, the stacked .local [world, 3])"""
    import torch
    ks = [_kwargs(_lanes(d, lo, hi), kw) for lo, hi in LS.bounds(split)]
    hs = [gmpe.compute_returns_begin(**k) for k in ks]
    stats = torch.stack([h.local for h in hs])
    for h in hs:
        gmpe.compute_returns_finish(h, stats)
    torch.cuda.synchronize()
    parts = [_read(k) for k in ks]
    return {n: np.concatenate([p[n] for p in parts], 1) for n in OUT_KEYS}, stats.cpu().numpy()


_RUNS = {}


def _runs(name, path):
    """Every device run of a case, made once and shared."""
    if (name, path) not in _RUNS:
        d, kw, adv, am, split, asc = _returns_arrays(name, path)
        _RUNS[name, path] = (_whole(d, kw),) + _sharded(d, kw, split) + (adv, am, split, asc)
    return _RUNS[name, path]


RETURNS_RUNS = [(n, p) for n in LS.RETURNS_CASES for p in LS.PATHS] + [("branch", "recurrence")]


@pytest.mark.parametrize("name,path", RETURNS_RUNS)
def test_sharded_returns_are_the_unsharded_bits_and_one_global_pair(name, path):
    whole, sh, stats, adv, am, split, asc = _runs(name, path)
    for k in ("returns", "value_preds", "advantages"):
        assert R._same_bits(sh[k], whole[k]), "%s %s: %s differs from the unsharded call" % (name, path, k)
    assert R._same_bits(sh["advantages"], adv), "%s %s: the raw advantages are not the expected ones" % (name, path)
    for (lo, hi), row in zip(LS.bounds(split), stats):                 # .local: the shard's count, and an idle shard's n = 0
        keep = (am[:-1, lo:hi] != 0) & ~np.isnan(adv[:, lo:hi])
        assert row[0] == keep.sum(), (name, path, lo, hi)
    if "idle" in name:
        assert stats[-1, 0] == 0
    pairs = R.candidate_pairs(*R.stats64(adv, am))
    m, d = LS.emulate_returns(adv, am, split, asc)
    want = R.pair_offsets(m, d, pairs)
    got = R.match_pair(_bits(sh["advantages"]), _bits(sh["normalized"]), pairs)
    print("%s %s: device (dm, dd) = %r, host emulation %r" % (name, path, got, want))
    assert want is not None
    assert got is not None, "%s %s: no candidate pair reproduces the normalised advantages of all shards" % (name, path)
    assert got == want, "%s %s: inside the candidates, but not where the merge order lands on the host" % (name, path)
    assert R._same_bits(sh["normalized"], R.normalize32(sh["advantages"], m, d))          # every shard, the same pair
    if name.startswith("nan"):
        assert (np.isnan(sh["normalized"]) == np.isnan(adv)).all()


@pytest.mark.parametrize("name,path", [("offset-65+65", "advantages"), ("offset-65+65", "recurrence"), ("nan-65+65", "advantages"), ("branch", "recurrence")])
def test_returns_world_1_is_the_existing_call_bit_for_bit(name, path):
    d, kw, adv, am, split, asc = _returns_arrays(name, path)
    whole = _runs(name, path)[0]
    one, stats = _sharded(d, kw, (adv.shape[1],))
    assert stats.shape == (1, 3)
    for k in OUT_KEYS:
        assert R._same_bits(one[k], whole[k]), (name, path, k)
    import torch
    k = _kwargs(d, kw)                                                   # in place: `normalized` is `advantages`
    k["normalized"] = k["advantages"]
    h = gmpe.compute_returns_begin(**k)
    gmpe.compute_returns_finish(h, h.local.reshape(1, 3))
    with pytest.raises(RuntimeError, match="already called"):
        gmpe.compute_returns_finish(h, h.local.reshape(1, 3))
    torch.cuda.synchronize()
    assert R._same_bits(k["advantages"].cpu().numpy().reshape(adv.shape), whole["normalized"])


@pytest.mark.parametrize("path", LS.PATHS)
def test_plus_minus_100_shards_get_the_global_pair_not_their_own(path):
    """Shards with means near +100 and -100: what either would compute alone is far from the global statistics, so APPLY must have read `all`."""
    whole, sh, stats, adv, am, split, asc = _runs("pm100-90+40", path)
    d, kw = _returns_arrays("pm100-90+40", path)[:2]
    assert abs(stats[0, 1] - 100) < 1 and abs(stats[1, 1] + 100) < 1
    for lo, hi in LS.bounds(split):
        alone = _whole(_lanes(d, lo, hi), kw)
        assert R._same_bits(alone["advantages"], sh["advantages"][:, lo:hi])
        assert not R._same_bits(alone["normalized"], sh["normalized"][:, lo:hi])
        # alone, a shard's active entries normalise to about N(0, 1); with the global pair they all sit near (+-100 - 38) / 88 = 0.7 or -1.6
        assert np.median(np.abs(alone["normalized"] - sh["normalized"][:, lo:hi])[am[:-1, lo:hi] != 0]) > 0.1
    assert R._same_bits(sh["normalized"], R.normalize32(adv, *LS.emulate_returns(adv, am, split, asc)))


class _Rows(object):
    """An exchange inside one process: this shard's row is `local`, the other rows are given."""

    def __init__(self, rows, rank):
        self.rows, self.rank, self.world = rows, rank, rows.shape[0]

    def exchange(self, local):
        out = self.rows.clone()
        out[self.rank] = local
        return out


def test_one_call_forms_of_the_returns_run_begin_exchange_finish():
    import torch
    whole, sh, stats, adv, am, split, asc = _runs("unequal-1+128+64", "advantages")
    d, kw = _returns_arrays("unequal-1+128+64", "advantages")[:2]
    rows = torch.as_tensor(stats, device="cuda")
    for rank, (lo, hi) in enumerate(LS.bounds(split)):
        k = _kwargs(_lanes(d, lo, hi), kw)
        gmpe.engine.compute_returns(shards=_Rows(rows, rank), **k)
        torch.cuda.synchronize()
        assert R._same_bits(_read(k)["normalized"], sh["normalized"][:, lo:hi]), rank
    # the buffer: world 1 is normalized_advantages() itself
    from gmpe.engine import GmpeEngine
    from gmpe.rollout import DeviceRolloutBuffer
    T, N, A = 4, 6, 3
    eng = GmpeEngine(gmpe.make_config(num_envs=N, num_agents=A, episode_length=T, seed=5), device=0)
    args = types.SimpleNamespace(gamma=0.99, gae_lambda=0.95, use_gae=True, use_proper_time_limits=False, use_valuenorm=False, use_popart=False)
    buf = DeviceRolloutBuffer(eng, T, args=args, policy_fields="all", learner_fields="all")
    buf.warmup()
    g = torch.Generator(device=eng.device)
    g.manual_seed(0)
    for t in range(T):
        act = torch.randint(0, 25, (N * A, 1), generator=g, device=eng.device)
        buf.insert_step(act.view(N, A).to(torch.int32), values=torch.randn((N * A, 1), generator=g, device=eng.device), actions=act,
                        action_log_probs=torch.zeros((N * A, 1), device=eng.device), rnn_states=torch.zeros((N * A, 1, 64), device=eng.device),
                        rnn_states_critic=torch.zeros((N * A, 1, 64), device=eng.device))
    x = _Rows(torch.zeros((1, 3), dtype=torch.float64, device=eng.device), 0)
    ret = buf.compute_returns(torch.zeros(N, A, 1)).clone()
    assert torch.equal(buf.compute_returns(torch.zeros(N, A, 1), shards=x), ret)
    plain = buf.normalized_advantages().clone()
    assert torch.isfinite(plain).all() and torch.equal(buf.normalized_advantages(shards=x), plain)
    eng.check_errors()
    eng.close()


# ------------------------------------------------------------------------------------------------ PPO loss
from test_gpu_ppo_loss import _VN, _args, _check  # noqa: E402  (the unsharded suite's own ValueNorm stand-in and its bounds)

ROW_KEYS = ("action_log_probs", "imp_weights", "grad_logits", "grad_values")
SCALARS = ("policy_loss", "dist_entropy", "actor_loss", "value_loss", "ratio_mean")


def _shard_tensors(torch, inp, c, st):
    lg = torch.tensor(inp["logits"], device="cuda", requires_grad=True)
    vl = torch.tensor(inp["values"], device="cuda", requires_grad=True)
    f = {k: torch.tensor(inp[k], device="cuda") for k in P.COLS + ("actions", "available_actions")}
    return lg, vl, f, (_VN(torch, st) if c.use_valuenorm else None)


def _loss_sharded(torch, inp, c, st, split, reduce="sum"):
    """-> per shard: dict of the PPOLosses fields, the gradients through backward(), the stored gradients, the f64 out row, the ValueNorm state"""
    shards = []
    for lo, hi in LS.bounds(split):
        lg, vl, f, vn = _shard_tensors(torch, LS.rows_of(inp, lo, hi), c, st)
        shards.append((lg, vl, vn, gmpe.ppo_losses_begin(lg, vl, f, _args(c), vn)))
    stats = torch.stack([s[3].local for s in shards])
    got = []
    for lg, vl, vn, h in shards:
        res = gmpe.ppo_losses_finish(h, stats, reduce)
        res.actor_loss.backward()
        res.value_loss.backward()
        g = {k: getattr(res, k).detach().cpu().numpy() for k in res._fields}
        g.update(grad_logits=lg.grad.cpu().numpy(), grad_values=vl.grad.cpu().numpy(), stored_logits=h.call.grad_logits.cpu().numpy(),
                 stored_values=h.call.grad_values.cpu().numpy(), out=h.out.cpu().numpy(), state=vn.state() if vn else None, handle=h)
        got.append(g)
    return got, stats.cpu().numpy()


@pytest.mark.parametrize("case", LS.LOSS_CASES, ids=LS.loss_case_id)
def test_sharded_loss_matches_the_restatement_of_the_concatenated_minibatch(case):
    import torch
    inp, c, st, ref = LS.loss_case(case)
    got, stats = _loss_sharded(torch, inp, c, st, case[2])
    o = _lib.PPO_OUT.index
    for g, (lo, hi), row in zip(got, LS.bounds(case[2]), stats):
        assert row[3] == hi - lo and row[2] == inp["active_masks"][lo:hi].sum()
        assert g["out"][o("denom_policy")] == ref["denom_policy"] and g["out"][o("denom_value")] == ref["denom_value"]       # the global counts, exactly
        assert np.array_equal(_bits(g["grad_logits"]), _bits(g["stored_logits"])) and np.array_equal(_bits(g["grad_values"]), _bits(g["stored_values"]))
        for k in SCALARS:                                                # the float32 scalar is the f64 column rounded once
            assert np.array_equal(_bits(g[k]), _bits(np.float32(g["out"][o(k)])))
    whole = {k: np.concatenate([g[k] for g in got], 0) for k in ROW_KEYS}
    for k in SCALARS:
        whole[k] = sum(float(g["out"][o(k)]) for g in got)               # the shards' scalar rows add up to the scalars of the whole minibatch
    whole["state"] = got[0]["state"]
    _check(whole, ref, inp, c, LS.loss_case_id(case))
    if c.use_valuenorm:
        for g in got[1:]:                                                # every replica received the same update
            for k, v in got[0]["state"].items():
                assert np.array_equal(_bits(v), _bits(g["state"][k])), k
    if case[3] == "one_active" and c.use_policy_active_masks:
        lo, hi = LS.bounds(case[2])[1]
        assert (whole["grad_logits"][lo:hi] == 0).all() and np.isfinite(whole["grad_values"]).all()
        assert got[1]["out"][o("policy_loss")] == 0 and np.isfinite(got[1]["out"]).all()


@pytest.mark.parametrize("case", [c for c in LS.LOSS_CASES if c[3] == "pm100"], ids=LS.loss_case_id)
def test_plus_minus_100_returns_need_the_exchange(case):
    """Returns near +100 in shard 0 and near -100 elsewhere: a shard's own batch means would move the ValueNorm state (and the normalised returns behind
    grad_values) far outside the bounds test_sharded_loss_matches... holds them to — shown here on the device by running each shard alone."""
    import torch
    inp, c, st, ref = LS.loss_case(case)
    got, _ = _loss_sharded(torch, inp, c, st, case[2])
    off = []
    for g, (lo, hi) in zip(got, LS.bounds(case[2])):
        lg, vl, f, vn = _shard_tensors(torch, LS.rows_of(inp, lo, hi), c, st)
        gmpe.ppo_losses(lg, vl, f, _args(c), vn)
        alone = vn.state()["running_mean"].reshape(-1)[0]
        off.append(abs(float(alone) - float(g["state"]["running_mean"].reshape(-1)[0])) / LS.state_tolerance(inp, "running_mean"))
    print("%s: a shard alone moves running_mean by %s tolerances" % (LS.loss_case_id(case), ["%.1f" % x for x in off]))
    assert off[0] > 5, off                                               # the +100 shard is far from the global mean at either split


@pytest.mark.parametrize("fam,K", [(f, K) for f in LS.FAMILIES for K in LS.LOSS_KS])
def test_loss_world_1_is_the_existing_call_bit_for_bit(fam, K):
    import torch
    inp, c, st, ref = LS.loss_case((fam, K, LS.LOSS_SPLITS[0], None))
    (one,), stats = _loss_sharded(torch, inp, c, st, (LS.ROWS,))
    assert stats.shape == (1, 4)
    lg, vl, f, vn = _shard_tensors(torch, inp, c, st)
    res = gmpe.ppo_losses(lg, vl, f, _args(c), vn)
    res.actor_loss.backward()
    res.value_loss.backward()
    for k in res._fields:
        assert np.array_equal(_bits(getattr(res, k).detach().cpu().numpy()), _bits(one[k])), k
    assert np.array_equal(_bits(lg.grad.cpu().numpy()), _bits(one["grad_logits"])) and np.array_equal(_bits(vl.grad.cpu().numpy()), _bits(one["grad_values"]))
    if vn:
        for k, v in vn.state().items():
            assert np.array_equal(_bits(v), _bits(one["state"][k])), k
    with pytest.raises(RuntimeError, match="already called"):
        gmpe.ppo_losses_finish(one["handle"], torch.zeros((1, 4), dtype=torch.float64, device="cuda"))


def test_plain_call_after_a_sharded_one_in_the_same_workspace_is_the_fresh_call_bit_for_bit():
    """The unsharded finish reads its row count from the header word the sharded APPLY also writes (there: the global count, 1030). One workspace
    tensor through both shards of 257 + 773, then through a plain call over the 257 rows: that call must leave what it leaves in a fresh workspace."""
    import torch
    case = ("off_vn", 5, LS.LOSS_SPLITS[0], None)
    inp, c, st, ref = LS.loss_case(case)
    bounds = LS.bounds(case[2])
    ws = torch.zeros(gmpe.ppo_loss.workspace_bytes(max(case[2])), dtype=torch.uint8, device="cuda")
    rows = torch.as_tensor(np.stack([LS.shard_sums(LS.rows_of(inp, lo, hi)) for lo, hi in bounds]), device="cuda")
    for rank, (lo, hi) in enumerate(bounds):
        lg, vl, f, vn = _shard_tensors(torch, LS.rows_of(inp, lo, hi), c, st)
        res = gmpe.ppo_losses(lg, vl, f, _args(c), vn, workspace=ws, shards=_Rows(rows, rank))
        assert float(res.ratio_mean) != 0.0
    got = []
    for workspace in (ws, None):
        lg, vl, f, vn = _shard_tensors(torch, LS.rows_of(inp, *bounds[0]), c, st)
        res = gmpe.ppo_losses(lg, vl, f, _args(c), vn, workspace=workspace)
        res.actor_loss.backward()
        res.value_loss.backward()
        g = {k: getattr(res, k).detach().cpu().numpy() for k in res._fields}
        g.update(grad_logits=lg.grad.cpu().numpy(), grad_values=vl.grad.cpu().numpy(), **vn.state())
        got.append(g)
    used, fresh = got
    assert sorted(used) == sorted(fresh) and len(used) == len(SCALARS) + 2 + 2 + 3
    for k, v in fresh.items():
        assert np.isfinite(v).all(), k
        assert np.array_equal(_bits(used[k]), _bits(v)), k


def test_reduce_mean_is_sum_times_world_bit_for_bit():
    import torch
    case = ("on_vn", 25, (257, 773), None)
    inp, c, st, ref = LS.loss_case(case)
    s, _ = _loss_sharded(torch, inp, c, st, case[2], "sum")
    m, _ = _loss_sharded(torch, inp, c, st, case[2], "mean")
    for a, b in zip(s, m):
        for k in SCALARS + ("grad_logits", "grad_values"):
            assert np.array_equal(_bits(a[k] * np.float32(2)), _bits(b[k])), k
        for k in ("action_log_probs", "imp_weights"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        assert np.array_equal(a["out"], b["out"])                        # the f64 row stays the shard's contribution
        for k, v in a["state"].items():
            assert np.array_equal(_bits(v), _bits(b["state"][k])), k


def test_one_call_form_of_the_loss_runs_begin_exchange_finish():
    import torch
    case = ("on_vn", 5, (1, 256, 773), None)
    inp, c, st, ref = LS.loss_case(case)
    two_step, stats = _loss_sharded(torch, inp, c, st, case[2], "mean")
    rows = torch.as_tensor(stats, device="cuda")
    for rank, ((lo, hi), want) in enumerate(zip(LS.bounds(case[2]), two_step)):
        lg, vl, f, vn = _shard_tensors(torch, LS.rows_of(inp, lo, hi), c, st)
        res = gmpe.ppo_losses(lg, vl, f, _args(c), vn, shards=_Rows(rows, rank), reduce="mean")
        res.actor_loss.backward()
        res.value_loss.backward()
        for k in res._fields:
            assert np.array_equal(_bits(getattr(res, k).detach().cpu().numpy()), _bits(want[k])), (rank, k)
        assert np.array_equal(_bits(lg.grad.cpu().numpy()), _bits(want["grad_logits"])) and np.array_equal(_bits(vl.grad.cpu().numpy()), _bits(want["grad_values"]))


def test_popart_has_no_sharded_form():
    import torch
    lg = torch.zeros(6, 5, device="cuda")
    with pytest.raises(NotImplementedError, match="PopArt variant has no sharded form"):
        gmpe.ppo_losses_popart(lg, torch.zeros(6, 8, device="cuda"), {}, types.SimpleNamespace(use_popart=True), None,
                               shards=_Rows(torch.zeros((2, 4), dtype=torch.float64, device="cuda"), 0))


# ------------------------------------------------------------------------------------------------ graph capture
def test_both_phases_of_both_entries_capture_into_one_graph():
    """LOCAL, a device-to-device copy standing in for the exchange, and APPLY of the returns and of the loss, in one graph, world = 2: the other shard's row of
    `all` is fixed, this shard's row is copied from .local inside the graph. Two replays on changed inputs, each the eager call's bits."""
    import torch
    a, am, split = LS.returns_case("offset-65+65")
    T, L = a.shape[0], split[0]
    d, kw = _returns_arrays("offset-65+65", "advantages")[:2]
    ks = [_kwargs(_lanes(d, lo, hi), kw) for lo, hi in LS.bounds(split)]
    case = ("on_vn", 5, (257, 773), None)
    inp, c, st, ref = LS.loss_case(case)
    (lg, vl, f, vn), (lg1, vl1, f1, vn1) = (_shard_tensors(torch, LS.rows_of(inp, lo, hi), c, st) for lo, hi in LS.bounds(case[2]))
    # the other shard's rows, computed once
    other_r = gmpe.compute_returns_begin(**ks[1]).local.clone()
    other_l = gmpe.ppo_losses_begin(lg1, vl1, f1, _args(c), vn1).local.clone()
    all_r = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    all_l = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    all_r[1], all_l[1] = other_r, other_l
    ws = torch.empty(gmpe.ppo_loss.workspace_bytes(257), dtype=torch.uint8, device="cuda")
    names = ("running_mean", "running_mean_sq", "debiasing_term")
    k0 = ks[0]
    versions = [dict(ret=k0["returns"].clone(), logits=lg.detach().clone(), returns=f["returns"].clone())]
    versions.append(dict(ret=k0["returns"] * 0.5 + 3.0, logits=lg.detach() * 0.75, returns=f["returns"] + 1.5))
    versions.append(dict(ret=k0["returns"] * 2.0 - 50.0, logits=lg.detach() * 1.25 + 0.125, returns=f["returns"] * 0.5))

    def load(v):
        for k in names:
            getattr(vn, k).copy_(torch.tensor(np.asarray(st[k], np.float32)))
        k0["returns"].copy_(v["ret"])
        with torch.no_grad():
            lg.copy_(v["logits"])
        f["returns"].copy_(v["returns"])

    def call():
        h = gmpe.compute_returns_begin(**k0)
        all_r[0].copy_(h.local)
        gmpe.compute_returns_finish(h, all_r)
        g = gmpe.ppo_losses_begin(lg, vl, f, _args(c), vn, workspace=ws)
        all_l[0].copy_(g.local)
        res = gmpe.ppo_losses_finish(g, all_l)
        gl, = torch.autograd.grad(res.actor_loss, lg)
        gv, = torch.autograd.grad(res.value_loss, vl)
        return (k0["advantages"], k0["normalized"]) + tuple(getattr(res, k).detach() for k in res._fields) + (gl, gv, g.out) + tuple(getattr(vn, k) for k in names)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                           # warm-up on a side stream, as torch.cuda.graph wants
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = []
    for v in versions:
        load(v)
        eager.append([t.cpu().numpy().copy() for t in call()])
    assert not np.array_equal(eager[1][1], eager[2][1]) and not np.array_equal(eager[1][-3], eager[2][-3])       # the versions differ in both entries (normalized, running_mean)
    load(versions[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = call()
    for i, v in enumerate(versions):
        if i == 0:
            continue                                                     # replayed twice, on the two changed inputs
        load(v)
        graph.replay()
        torch.cuda.synchronize()
        for j, (x, y) in enumerate(zip(eager[i], static)):
            y = y.cpu().numpy()
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), "replay on version %d, output %d" % (i, j)
