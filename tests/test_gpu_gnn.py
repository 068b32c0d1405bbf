"""The policy's GNNBase on the device (gmpe.gnn_base, gmpe_gnn_forward / gmpe_gnn_backward) against the float64 restatement of tests/gnn_lib.py (the edge-list
formulation, torch autograd). err(a) = max|a - a64| / max(1, max|a64|); per array the device is held to err_dev <= 4 * err_ref + 2^-23, err_ref being the
error of the restatement's own float32 run on the CPU, capped at 1e-5 (tests/test_gnn_host.py asserts the cap for every case). Everything that is claimed
bit for bit is compared bit for bit. Nothing here is compared with PyG: torch_geometric is not installed where these tests were written."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gmpe
import gnn_lib as G
from gmpe import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BITS = (65, 7, G.ACTOR, False)                          # the case of the bit claims
MANY = 65 * 77                                          # graphs of E = 6: 1252 tiles of four over 256 workgroups, whose partial sums the finish adds


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def device_base(key):
    return G.build(G.CONFIGS[key]).to(DEV)


def run(key, x, adj, ids, gf, workspace=None):
    """gmpe.gnn_base + torch.autograd.grad of sum(features * gf) over every parameter -> {name: float32 array}, named as gnn_lib.run names them"""
    base = device_base(key)
    ps = dict(base.named_parameters())
    f = gmpe.gnn_base(x.to(DEV), adj.to(DEV), ids.to(DEV), base, workspace=workspace)
    grads = torch.autograd.grad((f * gf.to(DEV)).sum(), list(ps.values()))
    torch.cuda.synchronize()
    res = {"features": f.detach().cpu().numpy()}
    res.update({"grad_" + k: g.cpu().numpy() for k, g in zip(ps, grads)})
    return res


@functools.lru_cache(maxsize=None)
def device_run(case):
    n, E, key, special = case
    return run(key, *G.inputs(n, E, key, special)[:4])


def check(got, t64, e_ref, what):
    for k in t64:
        e_dev = G.err(got[k], t64[k])
        print("%s %-44s err_ref %.3g err_dev %.3g bound %.3g" % (what, k, e_ref[k], e_dev, G.bound(e_ref[k])))
    for k in t64:
        assert e_ref[k] <= G.CAP, (what, k, e_ref[k])
        assert G.err(got[k], t64[k]) <= G.bound(e_ref[k]), (what, k, G.err(got[k], t64[k]), e_ref[k])


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_forward_and_backward_agree_with_the_float64_restatement(case):
    """the shipped actor (node) and critic (mean) weights over the shapes, max and add at 65 x 6, the F = 8 checkpoint, the random configurations (heads 1 and
    4, gnn_layer_N 0, embed_layer_N 0 and 2, Tanh, no LayerNorm, F = 8 and 16), and the written edge cases inside one batch.

    Measured (one run, one MI355X): all 964 arrays hold; the worst err_dev / bound is 0.70, the mean err_dev / err_ref over the 790 arrays with
    err_ref > 1e-7 is 0.57 and none exceeds 3."""
    n, E, key, special = case
    t64, e_ref = G.truth(n, E, key, special)
    got = device_run(case)
    assert sorted(got) == sorted(t64)
    check(got, t64, e_ref, G.case_id(case))


# ---------------------------------------------------------------------------------------------- 2
def test_a_graph_does_not_depend_on_its_batch_or_its_place():
    n, E, key, _ = BITS
    x, adj, ids, gf, _ = G.inputs(n, E, key)
    full = device_run(BITS)["features"]
    base = device_base(key)
    with torch.no_grad():
        a = 0
        for m in (1, 5, 59):                            # the 65 graphs as calls of 1, 5 and 59, and every graph alone at the head of a call
            f = gmpe.gnn_base(x[a:a + m].to(DEV), adj[a:a + m].to(DEV), ids[a:a + m].to(DEV), base).cpu().numpy()
            assert same(f, full[a:a + m]), "graphs %d .. %d" % (a, a + m - 1)
            a += m
        assert a == n
        back = gmpe.gnn_base(x.flip(0).to(DEV), adj.flip(0).to(DEV), ids.flip(0).to(DEV), base).cpu().numpy()
        assert same(back[::-1], full)


def test_no_grad_forward_is_the_training_forward_and_takes_no_workspace():
    n, E, key, _ = BITS
    x, adj, ids, gf, _ = G.inputs(n, E, key)
    full = device_run(BITS)["features"]
    base = device_base(key)
    args = (x.to(DEV), adj.to(DEV), ids.to(DEV))
    with torch.no_grad():
        f = gmpe.gnn_base(*args, base)
        g = gmpe.gnn_base(*args, base, workspace=torch.empty((8,), dtype=torch.uint8, device=DEV))          # a workspace it does not need is not used
    assert not f.requires_grad and f.grad_fn is None and same(f.cpu().numpy(), full) and same(g.cpu().numpy(), full)
    frozen = G.build(G.CONFIGS[key]).to(DEV).requires_grad_(False)                  # nothing requires a gradient: the forward-only plan as well
    f = gmpe.gnn_base(*args, frozen)
    assert not f.requires_grad and same(f.cpu().numpy(), full)
    for ids2 in (ids.to(torch.int32), ids.to(torch.float32), ids.view(n, 1)):       # the id's types and shapes
        with torch.no_grad():
            assert same(gmpe.gnn_base(args[0], args[1], ids2.to(DEV), base).cpu().numpy(), full)


def test_the_gradients_are_deterministic_and_a_reused_workspace_does_not_show():
    n, E, key, _ = BITS
    I = G.inputs(n, E, key)[:4]
    full = device_run(BITS)
    nbytes = gmpe.gnn_workspace_bytes(n, E, G.CONFIGS[key]["F"])
    assert nbytes == G.geometry(n, E)["workspace"]
    ws = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    a, b = run(key, *I, workspace=ws), run(key, *I)
    for k in full:
        assert same(a[k], full[k]) and same(b[k], full[k]), k
    assert bool((ws[nbytes:] == 0xFF).all())            # nothing is written past gmpe_gnn_workspace_bytes
    with pytest.raises(ValueError, match="workspace must be a contiguous uint8 tensor of at least %d bytes" % nbytes):
        run(key, *I, workspace=ws[:nbytes - 8])


@pytest.mark.parametrize("key", [G.ACTOR, G.CRITIC])
def test_the_shared_adjacency_gives_the_materialised_forms_bits(key):
    envs, S, E = 7, 3, 6
    x, adj, ids, gf, _ = G.inputs(envs * S, E, key)
    compact = adj[::S].contiguous()                     # one matrix per env, serving its S consecutive rows
    full = run(key, x, compact.repeat_interleave(S, 0), ids, gf)
    got = run(key, x, compact, ids, gf)
    for k in full:
        assert same(got[k], full[k]), k
    with pytest.raises(ValueError, match="adj must have shape"):
        run(key, x, adj[:4], ids, gf)


# ---------------------------------------------------------------------------------------------- 3
GUARD = 3                                               # rows (elements) behind every output, which the kernels must leave alone


def c_call(case, backward=True, fill=0, stream=None):
    """gmpe_gnn_forward (+ gmpe_gnn_backward, twice) through ctypes with caller-owned buffers -> {name: array}; fill: the byte the workspace holds before"""
    from gmpe import gnn as W
    lib = _lib.load()
    n, E, key, special = case
    x, adj, ids, gf, _ = G.inputs(n, E, key, special)
    base = device_base(key)
    names, ps, meta = W._base_params(base)
    ps = [p.detach().contiguous() for p in ps]
    xd, ad, idd = x.to(DEV), adj.to(DEV), ids.to(DEV).to(torch.int32)
    shape = (n, E, x.shape[2], 1, int(ps[0].shape[0]), int(ps[0].shape[1]))
    p = W._plan(shape, meta, xd, ad, idd, ps)
    nan = float("nan")
    f = torch.full((n + GUARD, G.C), nan, device=DEV)
    p.features = f.data_ptr()
    st = C.c_void_p((stream or torch.cuda.current_stream(torch.device(DEV))).cuda_stream)
    _lib.check(lib.gmpe_gnn_forward(0, C.byref(p), st), "gmpe_gnn_forward")
    torch.cuda.synchronize()
    a = f.cpu().numpy()
    assert np.isnan(a[n:]).all(), "rows past the end of features were written"
    res = {"features": a[:n]}
    if backward:
        nbytes = C.c_size_t()
        _lib.check(lib.gmpe_gnn_workspace_bytes(C.byref(p), 1, C.byref(nbytes)), "gmpe_gnn_workspace_bytes")
        nbytes = nbytes.value
        assert nbytes == gmpe.gnn_workspace_bytes(n, E, x.shape[2], meta[0], meta[1], meta[2], shape[4], shape[5])
        ws = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device=DEV)
        gfd = gf.to(DEV)
        gps = [torch.full((t.numel() + GUARD,), nan, device=DEV) for t in ps]
        p.workspace, p.workspace_bytes, p.grad_features, p.features = ws.data_ptr(), nbytes, gfd.data_ptr(), None
        W._fill(p, meta, meta[5], meta[2], meta[1], gps, "grad_")
        for rep in range(2):                            # backward may be repeated on one plan: fresh outputs, the same bits
            _lib.check(lib.gmpe_gnn_backward(0, C.byref(p), st), "gmpe_gnn_backward")
            if rep == 0:
                torch.cuda.synchronize()
                first = [g.clone() for g in gps]
                for g in gps:
                    g.fill_(nan)
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == fill).all()), "bytes past the workspace were written"
        by_tensor = {id(t): k for k, t in base.named_parameters()}
        for name, like, g, g1 in zip(names, W._base_params(base)[1], gps, first):
            a = g.cpu().numpy()
            assert same(a, g1.cpu().numpy()), "the second backward call differs: " + name
            assert np.isnan(a[like.numel():]).all(), "elements past the end of grad %s were written" % name
            res["grad_" + by_tensor[id(like)]] = a[:like.numel()].reshape(tuple(like.shape))
    return res


@pytest.mark.parametrize("case", [BITS, (8, 9, G.CRITIC, True), (12, 44, G.cfg_key(G._RANDOM[-1]), False), (9, 11, G.cfg_key(G._RANDOM[7]), False),
                                  (9, 11, G.cfg_key(G._RANDOM[2]), False)], ids=G.case_id)
def test_the_c_entries_give_the_wrappers_bits_and_stay_inside_their_outputs(case):
    a, b = device_run(case), c_call(case)
    assert sorted(a) == sorted(b)
    for k in a:
        assert same(a[k], b[k]), k


def test_the_workspaces_old_contents_do_not_show_and_a_side_stream_works():
    full = device_run(BITS)
    ones = c_call(BITS, fill=0xFF)
    fwd = c_call(BITS, backward=False)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = c_call(BITS, stream=side)
        wrapped = run(BITS[2], *G.inputs(*BITS[:3])[:4])        # the wrapper launches on the current stream
    for k in full:
        assert same(ones[k], full[k]) and same(other[k], full[k]) and same(wrapped[k], full[k]), k
    assert same(fwd["features"], full["features"])


def test_bad_entity_types_and_ids_read_nothing_out_of_bounds():
    """types and ids far outside their ranges are clamped: the run ends clean, the untouched graphs keep their bits, and the clamped rows are the rows of
    the clamped values"""
    n, E, key, _ = BITS
    x, adj, ids, gf, _ = G.inputs(n, E, key)
    full = device_run(BITS)["features"]
    base = device_base(key)
    x2, ids2 = x.clone(), ids.clone()
    x2[3, :, -1] = torch.tensor([1e9, -1e9, float("nan"), 77.0, -3.0, 4.0, 2.5][:E])
    ids2[5], ids2[6] = 10 ** 6, -(10 ** 6)
    x3, ids3 = x2.clone(), ids2.clone()
    x3[3, :, -1] = torch.tensor([3.0, 0.0, 0.0, 3.0, 0.0, 3.0, 2.0][:E])
    ids3[5], ids3[6] = E - 1, 0
    with torch.no_grad():
        got = gmpe.gnn_base(x2.to(DEV), adj.to(DEV), ids2.to(DEV), base).cpu().numpy()
        want = gmpe.gnn_base(x3.to(DEV), adj.to(DEV), ids3.to(DEV), base).cpu().numpy()
    keep = [g for g in range(n) if g not in (3, 5, 6)]
    assert same(got[keep], full[keep]) and same(got, want) and np.isfinite(got).all()


# ---------------------------------------------------------------------------------------------- 4
def test_a_workgroup_with_several_tiles_and_a_finish_over_several_partials():
    """5005 graphs of E = 6: every workgroup of backward owns four or five tiles of four graphs, and the finish adds 256 partial rows. With the loss weight on
    the last graph alone, every other graph contributes exact zeros, the last graph's float32 chains are those of the one-graph call and the double sums
    add zeros to them: every parameter gradient has the one-graph call's bits. The forward of every graph has the bits of its own call's."""
    key, E = G.ACTOR, 6
    geo = G.geometry(MANY, E)
    assert geo["W_bwd"] == 4 and geo["tiles_bwd"] == 1252 and geo["blocks_bwd"] == 256 and geo["tiles_fwd"] > geo["blocks_fwd"]
    x, adj, ids, gf, _ = G.inputs(65, E, key)
    reps = MANY // 65
    X, A, I = (t.repeat((reps,) + (1,) * (t.dim() - 1))[:MANY] for t in (x, adj, ids))
    last = MANY - 1
    W = torch.zeros((MANY, G.C))
    W[last] = gf[0]
    many = run(key, X, A, I, W)
    one = run(key, X[last:], A[last:], I[last:], W[last:])
    small = run(key, x, adj, ids, gf)
    assert same(many["features"][:65], small["features"]) and same(many["features"][last:], one["features"])
    assert same(many["features"][65 * (reps - 2):65 * (reps - 1)], small["features"])
    assert sum(np.abs(v).max() > 0 for v in one.values()) > len(one) // 2         # the comparison is not one of zeros
    for k in one:
        if k != "features":
            assert same(many[k], one[k]), k
    # and with every graph weighted, against the truth of the 65 graphs, each of which appears 77 times: the accuracy rule
    t64, e_ref = G.truth(65, E, key)
    allw = run(key, X, A, I, gf.repeat((reps, 1))[:MANY])
    for k in t64:
        if k != "features":
            assert e_ref[k] <= G.CAP and G.err(allw[k] / 77.0, t64[k]) <= G.bound(e_ref[k]), (k, G.err(allw[k] / 77.0, t64[k]), e_ref[k])


# ---------------------------------------------------------------------------------------------- 5
class _Chain(torch.nn.Module):
    """GNNBase -> MLPBase(cat(obs, nbd)) -> RNNLayer, with the reference's attribute names"""

    def __init__(self, cfg, obs_dim):
        super().__init__()
        nn = torch.nn
        self.gnn_base = G.Base(cfg)
        self.base = nn.Module()
        self.base._use_feature_normalization = True
        self.base.feature_norm = nn.LayerNorm(obs_dim + G.C)
        self.base.mlp = nn.Module()
        self.base.mlp._layer_N = 1
        self.base.mlp.fc1 = nn.Sequential(nn.Linear(obs_dim + G.C, 64), nn.ReLU(), nn.LayerNorm(64))
        self.base.mlp.fc2 = nn.ModuleList([nn.Sequential(nn.Linear(64, 64), nn.ReLU(), nn.LayerNorm(64))])
        self.rnn = nn.Module()
        self.rnn._recurrent_N = 1
        self.rnn.rnn = nn.GRU(64, 64)
        self.rnn.norm = nn.LayerNorm(64)

    def torch_forward(self, obs, x, adj, ids, hxs, masks, L):
        dt = obs.dtype
        nbd = G.forward(self.gnn_base, x.to(dt), adj.to(dt), ids)
        f = self.base.feature_norm(torch.cat([obs, nbd], 1))
        f = self.base.mlp.fc2[0](self.base.mlp.fc1(f))
        Nb = hxs.shape[0]
        h, outs, m = hxs.transpose(0, 1), [], masks.view(L, 1, Nb, 1)
        for t in range(L):
            o, h = self.rnn.rnn(f.view(L, Nb, 64)[t:t + 1], h * m[t])
            outs.append(o)
        return self.rnn.norm(torch.cat(outs).reshape(L * Nb, 64)), h.transpose(0, 1)


def test_gnn_base_chained_into_mlp_base_and_rnn_layer():
    """gradients reach the three modules' parameters through the three nodes; against the same chain in torch on the CPU (the restatement, torch's Linear /
    LayerNorm / GRU), float64 for the truth and float32 for err_ref, at 6 steps x 5 rows of E = 7"""
    L, Nb, E, obs_dim = 6, 5, 7, 6
    cfg = G.CONFIGS[G.ACTOR]
    torch.manual_seed(11)
    chain = _Chain(cfg, obs_dim)
    chain.gnn_base.load_state_dict(G.build(cfg).state_dict())
    x, adj, ids, _, _ = G.inputs(L * Nb, E, G.ACTOR)
    obs, hxs = torch.randn(L * Nb, obs_dim), torch.rand(Nb, 1, 64) * 2 - 1
    masks = (torch.rand(L * Nb, 1) > 0.2).float()
    gf, gh = torch.randn(L * Nb, 64), torch.randn(Nb, 1, 64)

    def cpu(dt):
        net = _Chain(cfg, obs_dim)
        net.load_state_dict(chain.state_dict())
        net = net.to(dt)
        f, ho = net.torch_forward(obs.to(dt), x, adj, ids, hxs.to(dt), masks.to(dt), L)
        ((f * gf.to(dt)).sum() + (ho * gh.to(dt)).sum()).backward()
        res = {"features": f, "hxs_out": ho}
        res.update({"grad_" + k: p.grad for k, p in net.named_parameters()})
        return {k: v.detach().double().numpy() for k, v in res.items()}
    t64, r32 = cpu(torch.float64), cpu(torch.float32)
    e_ref = {k: G.err(r32[k], t64[k]) for k in t64}
    net = chain.to(DEV)
    nbd = gmpe.gnn_base(x.to(DEV), adj.to(DEV), ids.to(DEV), net.gnn_base)
    f, ho = gmpe.rnn_layer(gmpe.mlp_base((obs.to(DEV), nbd), net.base), hxs.to(DEV), masks.to(DEV), net.rnn)
    ((f * gf.to(DEV)).sum() + (ho * gh.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    got = {"features": f.detach().cpu().numpy(), "hxs_out": ho.detach().cpu().numpy()}
    got.update({"grad_" + k: p.grad.cpu().numpy() for k, p in net.named_parameters()})
    check(got, t64, e_ref, "gnn_base -> mlp_base -> rnn_layer")
