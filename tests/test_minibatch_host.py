"""CPU side of the PPO minibatch gather (include/gmpe.h gmpe_minibatch_gather; gmpe.minibatch; DeviceRolloutBuffer.feed_forward_generator /
recurrent_generator): the exported symbol, the plan struct layout, the argument checks of the C entry point and of the Python wrappers before any launch, and the
NumPy restatement of the sampler arithmetic and the two index maps (tests/minibatch_lib.py) against the reference's own yields; the byte-level form of that
restatement (gather_bytes) against the shaped one on the same yields, and the cases the kernel tests draw from it (KERNEL_CASES): which case tells which wrong
restatement from the right one, and what the cases cover."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_lib
import gmpe
from gmpe import _lib
import minibatch_lib as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "minibatch_generators.npz")


def test_symbol_is_exported_and_bound():
    assert "gmpe_minibatch_gather" in _lib.SYMBOLS and "gmpe_minibatch_gather" in abi_lib.exported()


def test_plan_struct_layout_matches_c_header():
    for P in (_lib.GmpeMbField, _lib.GmpeMinibatchPlan):
        assert abi_lib.layout(P) == abi_lib.mirror_layout(P)
    names = ("FEED_FORWARD", "RECURRENT", "ROW", "ENV_ROW", "CHUNK_HEAD", "TABLE_NODE", "TABLE_ADJ", "MAX_FIELDS")
    assert [abi_lib.constant("GMPE_MB_" + k) for k in names] == [getattr(_lib, "MB_" + k) for k in names]


def _plan(**kw):
    p = _lib.GmpeMinibatchPlan()
    p.mode, p.num_fields, p.T, p.N, p.A, p.L = _lib.MB_FEED_FORWARD, 1, 4, 3, 2, 1
    p.perm, p.perm_len, p.offset, p.rows = 0x10000, 24, 0, 8                  # fake device addresses: nothing may be touched before the checks pass
    f = p.fields[0]
    f.kind, f.row_bytes, f.slot_stride, f.src, f.dst = _lib.MB_ROW, 16, 3 * 2 * 16, 0x20000, 0x30000
    for k, v in kw.items():
        if k.startswith("f_"):
            setattr(f, k[2:], v)
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad", [
    dict(mode=7), dict(num_fields=0), dict(num_fields=_lib.MB_MAX_FIELDS + 1), dict(T=0), dict(N=0), dict(mode=_lib.MB_RECURRENT, L=0),
    dict(T=1 << 16, N=1 << 16, A=1), dict(perm=None), dict(perm=0x10004), dict(rows=0), dict(offset=-1), dict(offset=20),
    dict(f_kind=9), dict(f_src=None), dict(f_dst=None), dict(f_row_bytes=6), dict(f_row_bytes=0), dict(f_slot_stride=16),
    dict(f_kind=_lib.MB_CHUNK_HEAD), dict(f_dst=0x30002), dict(f_kind=_lib.MB_TABLE_NODE),
    dict(T=1 << 11, N=1 << 10, A=1 << 10, f_slot_stride=1 << 24),                                   # T * N * A exactly 2^31
    dict(perm_len=1 << 27, rows=1 << 27, f_row_bytes=1040, f_slot_stride=6 * 1040),                 # 2^27 rows of 65 units: rows * units above 2^31 - 1
])
def test_c_entry_point_refuses_bad_plans_before_any_device_call(bad):
    lib = _lib.load()
    assert lib.gmpe_minibatch_gather(None, 0, C.byref(_plan(**bad)), None) == -1
    assert lib.gmpe_last_error().decode().startswith("gmpe_minibatch_gather:")


def test_c_entry_point_checks_table_kinds_against_the_config():
    lib = _lib.load()
    cfg = gmpe.make_config(num_envs=3, num_agents=2, episode_length=4)
    E, W, F = cfg.num_entities, cfg.entity_table_width, cfg.node_feats
    ok = dict(f_kind=_lib.MB_TABLE_ADJ, f_row_bytes=E * E * 4, f_slot_stride=3 * W * 8)
    assert lib.gmpe_minibatch_gather(None, 0, C.byref(_plan(**ok)), None) == -1                        # no config
    for bad in (dict(f_row_bytes=E * E * 4 + 4), dict(f_slot_stride=3 * W * 8 - 8), dict(f_src=0x20004), dict(A=3),
                dict(f_kind=_lib.MB_TABLE_NODE, f_row_bytes=E * E * 4), dict(f_kind=_lib.MB_TABLE_NODE, f_row_bytes=E * F * 4, f_dst=0x30004)):
        assert lib.gmpe_minibatch_gather(C.byref(cfg), 0, C.byref(_plan(**dict(ok, **bad))), None) == -1, bad
    assert lib.gmpe_minibatch_gather(None, 0, None, None) == -1


def test_python_wrappers_refuse_bad_arguments_before_any_launch():
    from gmpe.minibatch import Gather, device_perm, feed_forward_sizes
    cfg = gmpe.make_config(num_envs=3, num_agents=2, episode_length=4)
    T, N, A, E = 4, 3, 2, cfg.num_entities
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    arrays = dict(obs=z(T + 1, N, A, cfg.obs_dim), agent_id=z(T + 1, N, A, 1, dt=torch.int32), masks=z(T + 1, N, A, 1), active_masks=z(T + 1, N, A, 1),
                  node_obs=z(T + 1, N, A, E, cfg.node_feats), adj=z(T + 1, N, E, E))
    with pytest.raises(ValueError, match="CUDA"):
        Gather(cfg, arrays)                                                     # host tensors: no CPU fallback
    for k, v in (("obs", None), ("masks", None)):
        with pytest.raises(ValueError):
            Gather(cfg, dict(arrays, **{k: v}))
    with pytest.raises(ValueError, match="unknown"):
        Gather(cfg, dict(arrays, values=z(1)))
    with pytest.raises(ValueError, match="agents"):
        Gather(gmpe.make_config(num_envs=3, num_agents=3, episode_length=4), arrays)
    with pytest.raises(AssertionError, match=r"PPO requires the number of processes \(3\) \* number of steps \(4\) \* number of agents \(2\) = 24"):
        feed_forward_sizes(T, N, A, num_mini_batch=25)
    with pytest.raises(ValueError):
        device_perm(torch.arange(5), 6, "cpu")                                  # wrong length
    with pytest.raises(ValueError):
        device_perm(torch.arange(6, dtype=torch.int32), 6, "cpu")              # wrong dtype
    with pytest.raises(ValueError, match="lie in"):
        device_perm(torch.tensor([0, 1, 2, 3, 4, 6]), 6, "cpu")
    with pytest.raises(ValueError):
        device_perm("host", 6, "cpu")


def test_buffer_methods_refuse_bad_learner_arrays_and_the_naive_generator():
    from gmpe.rollout import DeviceRolloutBuffer
    b = DeviceRolloutBuffer.__new__(DeviceRolloutBuffer)                       # no engine needed for the checks
    b.T, b.engine = 4, type("E", (), dict(N=3, A=2, device=torch.device("cpu")))()
    b.obs = b.agent_id = b.masks = b.active_masks = b.value_preds = b.returns = b.available_actions = b.entity_table = None
    b._node_obs, b._adj = torch.zeros(1), torch.zeros(1)
    with pytest.raises(ValueError, match="rnn_states"):
        b.minibatch_arrays(dict(rnn_states=torch.zeros(4, 3, 2, 1, 8)))        # T, not T+1 slots
    with pytest.raises(ValueError, match="actions"):
        b.minibatch_arrays(dict(actions=torch.zeros(5, 3, 2, 1)))
    with pytest.raises(ValueError, match="unknown"):
        b.minibatch_arrays(dict(values=torch.zeros(5, 3, 2, 1)))
    with pytest.raises(ValueError, match="advantages"):
        b._advantages(torch.zeros(5, 3, 2, 1))
    with pytest.raises(NotImplementedError, match="IndexError"):
        b.naive_recurrent_generator(torch.zeros(4, 3, 2, 1), 2)


def test_numpy_restatement_equals_the_reference_bit_for_bit():
    g = np.load(GOLD)
    T, N, A = int(g["T"]), int(g["N"]), int(g["A"])
    inp = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    assert "IndexError" in str(g["naive_error"])
    seen_rec_cross = left_chunks = False
    for case in g["cases"]:
        case = str(case)
        perm, nmb, L = g[case + "_perm"], int(g[case + "_num_mini_batch"]), int(g[case + "_data_chunk_length"])
        central, avail = bool(g[case + "_centralized"]), bool(g[case + "_avail"])
        arrays = dict(inp, available_actions=inp["available_actions"] if avail else None)
        if bool(g[case + "_recurrent"]):
            sampler = M.rec_sampler(T, N, A, nmb, L)
            assert T % L and (N * T * A) % L, case                            # chunks cross agents / envs; samples left over
            left_chunks |= bool((N * T * A // L) % nmb)
        else:
            sampler = M.ff_sampler(T, N, A, nmb)
        assert len(sampler) == int(g[case + "_num_batches"])
        for b, (off, rows) in enumerate(sampler):
            if bool(g[case + "_recurrent"]):
                (t, n, a), heads = M.rec_samples(perm, off, rows, T, N, A, L)
                seen_rec_cross |= bool((np.diff(n) != 0).any() or (np.diff(a.reshape(L, -1), axis=0) != 0).any())
                o = M.gather(arrays, t, n, a, central, heads)
            else:
                o = M.gather(arrays, *M.ff_samples(perm, off, rows, T, N, A), central)
            for k in M.NAMES:
                ref = g["%s_%d_%s" % (case, b, k)]
                if bool(g["%s_%d_%s_none" % (case, b, k)]):
                    assert o[k] is None, (case, b, k)
                    continue
                assert o[k].dtype == ref.dtype and o[k].shape == ref.shape and np.array_equal(o[k], ref), (case, b, k)
    assert seen_rec_cross and left_chunks


def test_the_two_size_refusals_name_their_reason():
    lib = _lib.load()
    for bad, why in ((dict(T=1 << 11, N=1 << 10, A=1 << 10, f_slot_stride=1 << 24), "T * N * A must be below 2^31"),
                     (dict(perm_len=1 << 27, rows=1 << 27, f_row_bytes=1040, f_slot_stride=6 * 1040), "too many units")):
        assert lib.gmpe_minibatch_gather(None, 0, C.byref(_plan(**bad)), None) == -1
        assert why in lib.gmpe_last_error().decode(), bad
    ok = _plan(T=(1 << 11) - 1, N=1 << 10, A=1 << 10, f_slot_stride=1 << 24, f_row_bytes=6)          # 2^31 - 2^20 samples pass that check: refused for the row size
    assert lib.gmpe_minibatch_gather(None, 0, C.byref(ok), None) == -1 and "row_bytes" in lib.gmpe_last_error().decode()


def test_byte_level_constants_are_the_bindings():
    assert (M.FEED_FORWARD, M.RECURRENT, M.ROW, M.ENV_ROW, M.CHUNK_HEAD, M.MAX_FIELDS) == \
        (_lib.MB_FEED_FORWARD, _lib.MB_RECURRENT, _lib.MB_ROW, _lib.MB_ENV_ROW, _lib.MB_CHUNK_HEAD, _lib.MB_MAX_FIELDS)


def test_byte_level_restatement_equals_the_shaped_one_on_the_reference_yields():
    """gather_bytes on a contiguous image of the fixture's arrays == gather + ff_samples / rec_samples, which the test above pins to the reference"""
    g = np.load(GOLD)
    T, N, A = int(g["T"]), int(g["N"]), int(g["A"])
    inp = {k[3:]: np.ascontiguousarray(g[k]) for k in g.files if k.startswith("in_")}
    checked = 0
    for case in (str(c) for c in g["cases"]):
        perm, nmb, L = g[case + "_perm"], int(g[case + "_num_mini_batch"]), int(g[case + "_data_chunk_length"])
        central, avail, rec = bool(g[case + "_centralized"]), bool(g[case + "_avail"]), bool(g[case + "_recurrent"])
        arrays = dict(inp, available_actions=inp["available_actions"] if avail else None)
        share = M.ENV_ROW if central else M.ROW
        spec = [("share_obs", share, "obs"), ("share_agent_id", share, "agent_id")] + \
            [(k, M.CHUNK_HEAD if rec and k.startswith("rnn") else M.ROW, k) for k in M.NAMES if not k.startswith("share") and arrays[k] is not None]
        for off, rows in (M.rec_sampler(T, N, A, nmb, L) if rec else M.ff_sampler(T, N, A, nmb)):
            if rec:
                (t, n, a), heads = M.rec_samples(perm, off, rows, T, N, A, L)
                want = M.gather(arrays, t, n, a, central, heads)
            else:
                want = M.gather(arrays, *M.ff_samples(perm, off, rows, T, N, A), central)
            fields, cur = [], 256
            for name, kind, src in spec:                                       # destinations, 256 sentinel bytes between them
                x = arrays[src]
                rb = x[0, 0].nbytes if kind == M.ENV_ROW else x[0, 0, 0].nbytes
                n_out = rows if kind == M.CHUNK_HEAD or not rec else rows * L
                fields.append(dict(kind=kind, row_bytes=rb, slot_stride=x[0].nbytes, dst=cur))
                cur = -(-(cur + n_out * rb) // 256) * 256 + 256
            for f, (name, kind, src) in zip(fields, spec):                     # the arrays as they lie in memory: contiguous, exactly one slot apart
                f["src"], cur = cur, -(-(cur + arrays[src].nbytes) // 256) * 256
            image = np.full(cur, M.SENTINEL, dtype=np.uint8)
            for f, (name, kind, src) in zip(fields, spec):
                image[f["src"]:f["src"] + arrays[src].nbytes] = arrays[src].reshape(-1).view(np.uint8)
            plan = dict(mode=M.RECURRENT if rec else M.FEED_FORWARD, T=T, N=N, A=A, L=L if rec else 1, perm=perm, offset=off, rows=rows, fields=fields)
            out = M.gather_bytes(plan, image)
            expect = image.copy()
            for f, (name, kind, src) in zip(fields, spec):
                w = np.ascontiguousarray(want[name]).reshape(-1).view(np.uint8)
                assert w.size == M.out_rows(plan, kind) * f["row_bytes"], (case, name)
                expect[f["dst"]:f["dst"] + w.size] = w
                checked += 1
            assert np.array_equal(out, expect), (case, off)
    assert checked > 100


class _Narrow(M.Header):
    def entry(self, e):
        return e & 0xffffffff


class _LessEqual(M.Header):
    def in_range(self, e, n_valid):
        return (e >= 0) & (e <= n_valid)


class _Swapped(M.Header):
    def split(self, r, rows):
        return r // rows, r % rows


class _HeadLast(M.Header):
    def head_l(self, rows):
        return rows - 1


class _EnvAsSample(M.Header):
    def row_index(self, kind, n, a, A):
        return n * A + a


class _ExactSlot(M.Header):
    def stride(self, field, slot):
        return slot


class _FieldGreater(M.Header):
    def unwritten_prefix(self, plan, i):                                       # the field's first workgroup finds its predecessor's thread count and returns
        return M.BLOCK * M.unit_width(plan["fields"][i]) if i else 0


class _NoModN(M.Header):
    def ff_tna(self, j, T, N, A):
        return j // (N * A), j // A, j % A


class _CeilCount(M.Header):
    def valid_count(self, samples, L, recurrent):
        return -(-samples // L) if recurrent else samples


# wrong restatement -> (rules, a case that must tell it from the right one)
WRONG = {
    "range check after narrowing to 32 bits": (_Narrow(), "oor_ff"),
    "entry <= valid count": (_LessEqual(), "oor_ff"),
    "recurrent r % rows and r / rows swapped": (_Swapped(), "rec_L7"),
    "chunk heads at l = rows - 1": (_HeadLast(), "rec_LT"),
    "GMPE_MB_ENV_ROW addressed as a sample row": (_EnvAsSample(), "align_ff_env_row_16"),
    "slot_stride replaced by the exact slot": (_ExactSlot(), "widths_alone"),
    "fields matched to workgroups with >": (_FieldGreater(), "wl_255"),
    "n = j / A without % N": (_NoModN(), "single"),
    "valid chunk count ceil(T*N*A / L)": (_CeilCount(), "oor_rec"),
}


@pytest.fixture(scope="module")
def kernel_cases():
    built = []
    for case in M.KERNEL_CASES:
        plan, image = M.build_case(case)
        built.append((case["name"], plan, image, M.gather_bytes(plan, image)))
    assert len({b[0] for b in built}) == len(built)
    return built


def _inside(plan, image, trace, what):
    """every source byte read lies behind the destinations and inside the image; every permutation entry read exists"""
    assert plan["src0"] <= trace["src_min"] and trace["src_max"] <= image.size and trace["perm_max"] < len(plan["perm"]), (what, trace, image.size)


def test_every_wrong_restatement_is_told_by_a_named_case(kernel_cases):
    for what, (rules, named) in WRONG.items():
        told = []
        for name, plan, image, right in kernel_cases:
            trace = {}
            wrong = M.gather_bytes(plan, image, rules, trace)
            _inside(plan, image, trace, (what, name))                         # so the same mistake made in the kernel reads nothing outside the buffer
            if not np.array_equal(wrong, right):
                told.append(name)
        print("%-45s told by %d cases: %s" % (what, len(told), " ".join(told[:6])))
        assert named in told, (what, named, told)
    # the second case of the pairs the issue names twice
    by = {b[0]: b for b in kernel_cases}
    for what, named in (("range check after narrowing to 32 bits", "oor_rec"), ("chunk heads at l = rows - 1", "oor_rec"),
                        ("fields matched to workgroups with >", "wl_257_reversed"), ("recurrent r % rows and r / rows swapped", "wl_256")):
        _, plan, image, right = by[named]
        assert not np.array_equal(M.gather_bytes(plan, image, WRONG[what][0]), right), (what, named)


def test_kernel_cases_cover_widths_thread_totals_and_the_field_limit(kernel_cases):
    alone = {(q, w): [] for q in ("src", "dst", "slot_stride", "row_bytes") for w in (16, 8, 4)}
    totals, max_fields, between = set(), [], []
    for name, plan, image, right in kernel_cases:
        trace = {}
        assert np.array_equal(M.gather_bytes(plan, image, trace=trace), right)
        _inside(plan, image, trace, name)
        fields = plan["fields"]
        for f in fields:
            assert f["kind"] in (M.ROW, M.ENV_ROW, M.CHUNK_HEAD) and f["row_bytes"] in M.ROW_SIZES and (f["src"] | f["dst"] | f["slot_stride"]) % 4 == 0
            slot = f["row_bytes"] * (plan["N"] if f["kind"] == M.ENV_ROW else plan["N"] * plan["A"])
            assert f["slot_stride"] - slot in M.PADS and f["src"] % 256 in M.OFFSETS and f["dst"] % 256 in M.OFFSETS
            for q in ("src", "dst", "slot_stride", "row_bytes"):
                if all(f[o] % 16 == 0 for o in ("src", "dst", "slot_stride", "row_bytes") if o != q):
                    alone[(q, M.unit_width(f))].append(name)
            totals.add(M.field_threads(plan, f))
        # guards: at least 256 sentinel bytes before and behind every destination, and they are still there in the expected image
        for f in fields:
            end = f["dst"] + M.out_rows(plan, f["kind"]) * f["row_bytes"]
            assert (right[f["dst"] - 256:f["dst"]] == M.SENTINEL).all() and (right[end:end + 256] == M.SENTINEL).all() and end + 256 <= plan["src0"], name
        if len(fields) == M.MAX_FIELDS:
            max_fields.append(name)
        groups = [-(-M.field_threads(plan, f) // M.BLOCK) for f in fields]
        if any(groups[i] == 1 and groups[i - 1] > 1 and groups[i + 1] > 1 for i in range(1, len(fields) - 1)):
            between.append(name)
    assert all(alone.values()), {k: len(v) for k, v in alone.items()}
    assert {255, 256, 257} <= totals and 1 in totals and max(totals) > 16 * M.BLOCK
    assert "wl_255" in max_fields and "wl_255_reversed" in max_fields
    assert "wl_255" in between and "wl_255_reversed" in between
    assert any(len(b[1]["fields"]) == 1 for b in kernel_cases)
