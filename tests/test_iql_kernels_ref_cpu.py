"""The references of tests/iql_kernels_ref.py, tested themselves (no GPU): chained into one step they are iql_ref.RefIQL.grads and
.train in float64; the fixture conditions of the edge cases of tests/test_iql_kernel_edges_gpu.py hold by the reference alone (the rows
on each side of each kink, every "exactly at" input exact in float32, every integer-regime sum below 2^24); the float32 restatement of
the loss kernel's operations stays inside its bound; and every refusal of the m3pc_debug_iql_* hooks comes before any HIP call."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import iql_kernels_ref as K
import iql_ref as R
from iql_kernels_ref import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_lists_the_ten_ids_of_the_source():
    hdr = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    block = hdr[hdr.index("IQL-trainer kernel ids"):hdr.index("(end of the IQL-trainer kernel ids)")]
    ids = {int(n): k for n, k in re.findall(r"(\d+) (iql_[a-z0-9_]+_kernel(?:<\d>)?)", block)}
    assert sorted(ids) == list(range(1, 11))
    src = open(os.path.join(ROOT, "m3pc_amd", "csrc", "iql.hip")).read()
    kernels = set(re.findall(r"__global__ __launch_bounds__\([A-Z_0-9]+\) void (iql_[a-z0-9_]+_kernel)", src))
    assert len(kernels) == 9 and {k.split("<")[0] for k in ids.values()} == kernels
    assert sorted(int(n) for n in re.findall(r"M3PC_IQL_PICK\((\d+)\)", src)) == list(range(1, 11))
    # every launch of the file goes through a launcher that records its id
    assert src.count("hipLaunchKernelGGL(") == 10
    assert set(K.KID.values()) == set(ids)


# ------------------------------------------------------------------------------------------------ one step, kernel by kernel
PART = {0: ("vf", "v."), 1: ("qf", "q1."), 2: ("qf", "q2."), 3: ("actor", "net."), 4: ("q_target", "q1."), 5: ("q_target", "q2.")}


def _net(ref, t):
    part, pre = PART[t]
    p = ref.p[part]
    return [p[pre + f] for f in R.FIELDS]


def _chained_step(ref, batch, k):
    """ImplicitQLearning.train as the seven launches make it, every kernel by its own reference, in float64.  Returns the losses and
    the gradients by part and name, and moves `ref`'s parameters, moments and target."""
    hp = ref.hp
    s, a, r, s2, d = [np.asarray(x, np.float64) for x in batch]
    B, A = s.shape[0], a.shape[1]
    Bp = K.pad32(B)
    nets = [_net(ref, t) for t in range(6)]
    pass_net, H = [0, 0, 4, 5, 1, 2, 3], nets[0][1].shape[0]
    x, h1, h2, out7 = [], [], [], []
    for f, t in enumerate(pass_net):
        W1, b1, W2, b2, W3, b3 = nets[t]
        x.append(K.features64(s2 if f == 0 else s, ref.om, ref.os, a, W1.shape[1]))
        h1.append(K.layer_ref(x[f], W1, b1, K.pad32(W1.shape[1]))[0])
        h2.append(K.layer_ref(h1[f], W2, b2, H)[0])
        o = K.layer_ref(h2[f], W3, b3, H, "tanh" if t == 3 else "none")[0]
        out7.append(np.pad(o, ((0, 0), (0, K.OUTW - o.shape[1]))))
    L = K.loss_ref(out7, r[:, 0], d[:, 0], a, ref.p["actor"]["log_std"], F(hp["expectile"]), F(hp["beta"]), F(hp["discount"]), A)
    d3 = [L["dv"].v.numpy()[:, None], L["dq1"].v.numpy()[:, None], L["dq2"].v.numpy()[:, None], L["dz"].v.numpy()]
    grads = {"vf": {}, "qf": {}, "actor": {"log_std": L["gls"].v.numpy()}}
    for t in range(4):
        part, pre = PART[t]
        W1, b1, W2, b2, W3, b3 = nets[t]
        f = K.train_pass(t)
        d2 = K.delta_ref(d3[t], W3, h2[f], K.delta_K(2, W3.shape[0], H))[0]
        d1 = K.delta_ref(d2, W2, h1[f], H)[0]
        for name_w, name_b, dl, act in (("net.4.weight", "net.4.bias", d3[t], h2[f]), ("net.2.weight", "net.2.bias", d2, h1[f]), ("net.0.weight", "net.0.bias", d1, x[f])):
            gW, _, gb, _ = K.grad_ref(dl, act, Bp)
            grads[part][pre + name_w], grads[part][pre + name_b] = gW, gb
    lr = dict(vf=hp["v_lr"], qf=hp["q_lr"], actor=hp["actor_lr"])
    for part in ("vf", "qf", "actor"):
        step, sq = K.adam_scalars(k, lr[part], hp["max_steps"] if part == "actor" else None)
        for name, g in grads[part].items():
            K.adam64(ref.p[part][name], ref.m[part][name], ref.v[part][name], g, step, sq)
    tau = hp["tau"]
    for name in ref.p["q_target"]:
        ref.p["q_target"][name] = (1.0 - tau) * ref.p["q_target"][name] + tau * ref.p["qf"][name]
    return L["losses"].v.numpy(), grads


def test_the_kernel_references_chained_are_the_float64_step():
    case = "h64"
    state, om, os_ = R.make_state(case)
    mine, theirs = R.RefIQL(state, om, os_), R.RefIQL(state, om, os_)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    for k, batch in enumerate(R.make_batches(case, 2)):
        l_want, g_want = theirs.grads(batch)
        theirs.train(batch)
        l_got, g_got = _chained_step(mine, batch, k)
        assert rel(l_got, l_want) <= 1e-12, (l_got, l_want)
        for part in g_want:
            assert set(g_got[part]) == set(g_want[part])
            for name in g_want[part]:
                assert rel(g_got[part][name], g_want[part][name]) <= 1e-12, (k, part, name)
        for part in R.PARTS:
            for name in theirs.p[part]:
                assert rel(mine.p[part][name], theirs.p[part][name]) <= 1e-12, (k, part, name)
        for part in ("qf", "vf", "actor"):
            for name in theirs.m[part]:
                assert rel(mine.m[part][name], theirs.m[part][name]) <= 1e-12 and rel(mine.v[part][name], theirs.v[part][name]) <= 1e-12, (k, part, name)


# ------------------------------------------------------------------------------------------------ the fixture conditions
def test_the_constants_sit_where_the_cases_say():
    assert math.exp(float(K.LN100_LO)) <= 100.0 < math.exp(float(K.LN100_HI)) and K.LN100_HI == np.nextafter(K.LN100_LO, F(np.inf))
    assert float(K.LN100_LO) <= math.log(100.0) < float(K.LN100_HI)
    assert K.TINY_POS > 0 and K.TINY_POS / F(2) == 0 and K.TINY_POS.dtype == F
    assert all(F(v) == v for v in K.LOG_STD_EDGES) and math.frexp(K.LOSS_BETA)[0] == 0.5
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(F(120.0)))


@pytest.mark.parametrize("A,B", [(1, 1), (8, 33), (9, 1023), (32, 1024), (32, 33)])
def test_the_loss_case_has_rows_on_each_side_of_each_kink(A, B):
    c = K.loss_case(A, B, 5)
    o = c["out7"]
    assert np.isnan(o[:6, :, 1:]).all() and np.isnan(o[6, :, A:]).all() and np.isfinite(o[:6, :, 0]).all() and np.isfinite(o[6, :, :A]).all()
    adv = np.minimum(o[2, :, 0], o[3, :, 0]) - o[1, :, 0]
    assert adv.dtype == F
    arg = c["beta"] * adv
    L = K.loss_ref(o, c["reward"], c["done"], c["action"], c["log_std"], c["expectile"], c["beta"], c["gamma"], A)
    assert (np.abs(L["adv"].v.numpy() - adv.astype(np.float64)) <= L["adv"].e.numpy()).all() and np.array_equal(np.sign(L["adv"].v.numpy()), np.sign(adv))
    assert np.array_equal(L["adv"].v.numpy()[:9], adv[:9].astype(np.float64))   # the placed rows are exact differences
    if B > 1:
        assert adv[0] > 0 and adv[1] < 0
        assert adv[2] == 0 and not np.signbit(adv[2]) and adv[3] == 0 and np.signbit(adv[3])
        assert arg[4] == K.LN100_LO and arg[5] == K.LN100_HI and arg[6] == 120 and (c["beta"] * adv).dtype == F
        assert np.array_equal(arg.astype(np.float64), c["beta"].astype(np.float64) * adv.astype(np.float64))   # beta adv is exact
        assert c["done"][7] == 1 and c["done"][8] == 0
        w = L["wgt"].v.numpy()
        assert w[0] == w[2] == w[3] == float(F(0.7)) and abs(w[1] - (1 - float(F(0.7)))) < 1e-15
        ea = L["ea"]
        assert ea.v[6] == 100 and ea.e[6] == 0 and ea.v[5] == 100 and ea.e[5] > 0 and ea.v[4] < 100 and ea.v[4] + ea.e[4] > 100
        assert (adv > 0).sum() >= 3 and (adv < 0).sum() >= 3 and 0 < c["done"].sum() < B
    ls = c["log_std"]
    if A >= 5:
        assert tuple(float(v) for v in ls[:5]) == K.LOG_STD_EDGES and list(L["inside"][:5]) == [False, True, True, True, False]
        g = L["gls"].v.numpy()
        assert g[0] == 0 and g[4] == 0 and g[1] != 0 and g[3] != 0 and float(L["gls"].e[0]) == 0 and float(L["gls"].e[4]) == 0
    else:
        assert ls[0] == 2 and L["inside"][0] and L["gls"].v[0] != 0
    # the float32 restatement of every operation stays inside the operation's bound
    for key in ("dv", "dq1", "dq2", "dz"):
        ev = L[key]
        ratio = float(((ev.s.double() - ev.v).abs() / (ev.e + K.TINY)).max())
        assert ratio <= 1, (key, ratio)


@pytest.mark.parametrize("rows,Kdim,out", [(64, 64, 64), (1024, 256, 256), (1024, 64, 32)])
def test_integer_regime_sums_stay_below_2_24(rows, Kdim, out):
    x, W, b = K.product_inputs("int", rows, Kdim, out, 1)
    assert K.int_sum_max(x, W, b) < 2 ** 24 and np.array_equal(x, np.rint(x))
    # the gradient's chain is as long as the batch: deltas and activations of the same range
    assert K.int_sum_max(x.T, W.T[:, :rows] if W.shape[1] >= rows else np.resize(W, (out, rows))) < 2 ** 24
    s, s2, a, om, os_ = K.obs_inputs("int", rows, 40, 24, 2)
    f = K.features32(s, om, os_, a, 64)
    assert np.array_equal(f.astype(np.float64), K.features64(s, om, os_, a, 64)) and np.array_equal(2 * f, np.rint(2 * f)) and np.abs(f).max() <= 16
    assert K.int_sum_max(2 * f, W[:, :64] if W.shape[1] >= 64 else W) < 2 ** 24
    assert set(np.log2(os_)) <= {-1.0, 0.0, 1.0} and np.array_equal(om, np.rint(om))


def test_relu_edges_places_all_three():
    h = np.abs(np.random.RandomState(0).normal(size=(33, 64))).astype(F)
    z, nz, tp = K.relu_edges(h, 1)
    assert z.any() and nz.any() and tp.any() and not np.signbit(h[z]).any() and np.signbit(h[nz]).all() and (h[tp] == K.TINY_POS).all()
    d = np.ones((33, 1))
    out, bound = K.delta_ref(d, np.ones((1, 64)), h, 8)
    assert (out[z] == 0).all() and (out[nz] == 0).all() and (out[tp] == 1).all()


def test_adam_restatement_on_hand_computed_values():
    """g = 0 with v = 0 leaves everything; a g whose square underflows moves m and p and leaves v at 0; a step size of 0 leaves p."""
    p = np.array([1.0, 1.0, 1.0], F)
    g = np.array([0.0, 1e-25, 3.0], F)
    m1, v1 = K.adam_moments32(np.zeros(3, F), np.zeros(3, F), g)
    assert m1[0] == 0 and v1[0] == 0 and v1[1] == 0 and m1[1] == K.OMB1 * g[1] and v1[2] == (K.OMB2 * F(3)) * F(3)
    step, sq = K.adam_scalars(0, 3e-4)
    p1 = K.adam_param32(p, m1, v1, step, sq, 1e-8)
    assert p1[0] == 1 and p1[1] == 1 and abs(float(p1[2]) - (1 - 3e-4)) < 1e-7    # 1e-25 / 1e-8 is far below an ulp of 1
    assert np.array_equal(K.adam_param32(p, m1, v1, 0.0, sq, 1e-8), p)
    assert K.adam_scalars(1000, 3e-4, 1000)[0] == 0.0 and K.adam_scalars(500, 3e-4, 1000)[0] > 0
    assert np.array_equal(K.soft32(p, g, 1.0, 0.0), p) and np.array_equal(K.soft32(p, g, 0.0, 1.0), g)


# ------------------------------------------------------------------------------------------------ the hooks' refusals
def test_every_bad_argument_is_refused_before_any_hip_call():
    """The refusals make no HIP call: they return M3PC_EINVAL on a machine without a device (every pointer below is host memory the
    hooks never read)."""
    import iql_lab as IL
    try:
        lib = IL.lab()
    except Exception as e:  # no hipcc here: the lab library cannot be built
        pytest.skip(f"the lab library cannot be built: {e}")
    err = lib.m3pc_last_error
    buf = C.create_string_buffer(1 << 12)
    p = (C.addressof(buf) + 15) & ~15
    picked = (C.c_int * 2)(7, 7)
    pk = C.cast(picked, IL.pi)

    def refused(fn, a, word, what):
        a.picked = pk
        picked[0] = picked[1] = 7
        rc = getattr(lib, fn)(C.byref(a))
        assert rc == -1 and word in err(), (fn, what, rc, err())
        assert picked[0] == 0 and picked[1] == 0, what

    for fn in IL.HOOKS:
        assert getattr(lib, fn)(None) == -1 and b"null arguments" in err(), fn

    def args(**kw):
        a = IL.IqlArgs()
        for arr in (a.net, a.am, a.av):
            for n in arr:
                for f in IL.NET_FIELDS:
                    setattr(n, f, p)
                n.in_, n.out = 8, 1
        for f in ("log_std", "ls_m", "ls_v", "om", "os", "state", "action", "reward", "next_state", "done", "h1", "h2", "out", "d3", "d2", "d1"):
            setattr(a, f, p)
        a.B, a.H, a.S, a.A, a.npass, a.which = 4, 64, 6, 2, 2, 1
        for k, v in kw.items():
            o = a
            *path, leaf = k.split("__")
            for q in path:
                o = getattr(o, q) if not q.isdigit() else o[int(q)]
            setattr(o, leaf, v)
        return a

    FW, LO, DE, GR = "m3pc_debug_iql_forward", "m3pc_debug_iql_loss", "m3pc_debug_iql_delta", "m3pc_debug_iql_grad"
    for fn in (FW, LO, DE, GR):
        for H in (0, 32, 96, 512):
            refused(fn, args(H=H), b"hidden", f"hidden {H}")
        for B in (0, -1, 1025):
            refused(fn, args(B=B), b"B ", f"B {B}")
        for A in (0, 33):
            refused(fn, args(A=A), b"A ", f"A {A}")
        for S in (0, 65):
            refused(fn, args(S=S), b"S ", f"S {S}")
    # forward
    for w in (0, 4):
        refused(FW, args(which=w), b"layer", f"layer {w}")
    for n in (0, 8):
        refused(FW, args(npass=n), b"npass", f"npass {n}")
    refused(FW, args(pass_net=(C.c_int * 7)(0, 6)), b"pass_net", "network 6")
    refused(FW, args(pass_net=(C.c_int * 7)(-1, 0)), b"pass_net", "network -1")
    for f in ("om", "os", "h1", "state", "net__0__W1", "net__0__b1"):
        refused(FW, args(**{f: None}), b"null pointer", f"layer 1 without {f}")
    refused(FW, args(pass_next=(C.c_int * 7)(1, 0), next_state=None), b"null pointer", "a next-state pass without next_state")
    refused(FW, args(action=None), b"action is null", "in 8 > S 6 without action")
    for i in (0, 65, 9):
        refused(FW, args(net__0__in_=i), b"in ", f"in {i} (S + A = 8)")
    refused(FW, args(S=40, A=32, net__0__in_=65), b"in ", "in 65")
    refused(FW, args(net__0__b1=p + 4), b"off 16", "b1 unaligned")
    refused(FW, args(h1=p + 8), b"off 16", "h1 unaligned")
    for f in ("h1", "h2", "net__0__W2", "net__0__b2"):
        refused(FW, args(which=2, **{f: None}), b"null pointer", f"layer 2 without {f}")
        refused(FW, args(which=2, **{f: p + 4}), b"off 16", f"layer 2 with {f} unaligned")
    for f in ("h2", "out", "net__0__W3"):
        refused(FW, args(which=3, **{f: None}), b"null pointer", f"layer 3 without {f}")
        refused(FW, args(which=3, **{f: p + 4}), b"off 16", f"layer 3 with {f} unaligned")
    refused(FW, args(which=3, net__0__b3=None), b"null pointer", "layer 3 without b3")
    for o in (0, 33):
        refused(FW, args(which=3, net__0__out=o), b"out ", f"out {o}")
    # loss
    for f in ("out", "reward", "done", "action", "log_std", "ls_m", "ls_v", "d3"):
        refused(LO, args(**{f: None}), b"null pointer", f"loss without {f}")
    # delta
    for w in (0, 3):
        refused(DE, args(which=w), b"neither", f"L {w}")
    for L, fs in ((2, ("d3", "h2", "d2", "net__3__W3")), (1, ("d2", "h1", "d1", "net__2__W2"))):
        for f in fs:
            refused(DE, args(which=L, **{f: None}), b"null pointer", f"delta {L} without {f}")
            if "net" not in f:
                refused(DE, args(which=L, **{f: p + 4}), b"off 16", f"delta {L} with {f} unaligned")
    for o in (0, 33):
        refused(DE, args(which=2, net__1__out=o), b"out ", f"out {o}")
    # grad
    for f in ("d1", "d2", "d3", "h1", "h2", "om", "os", "state", "net__5__b3", "net__4__W1", "am__3__W2", "av__0__b1", "net__2__W3"):
        refused(GR, args(**{f: None}), b"null pointer", f"grad without {f}")
    refused(GR, args(action=None), b"action is null", "grad without action")
    refused(GR, args(pass_next=(C.c_int * 7)(0, 1), next_state=None), b"null pointer", "grad reading next_state")
    for i in (0, 65, 9):
        refused(GR, args(net__2__in_=i), b"in ", f"in {i}")
    for o in (0, 33):
        refused(GR, args(net__3__out=o), b"out ", f"out {o}")

    # eval_out, copy
    E, Cp = lib.m3pc_debug_iql_eval_out, lib.m3pc_debug_iql_copy
    for bad, what in (((None, 32, 4, 0, 1, p), "null out"), ((p, 32, 4, 0, 1, None), "null dst"), ((p, 32, 0, 0, 1, p), "rows 0"),
                      ((p, 2048, 1025, 0, 1, p), "rows 1025"), ((p, 32, 33, 0, 1, p), "Bp < rows"), ((p, 40, 33, 0, 1, p), "Bp % 32"),
                      ((p, 32, 4, 0, 0, p), "width 0"), ((p, 32, 4, 1, 33, p), "width 33")):
        picked[0] = picked[1] = 7
        assert E(*bad, None, pk) == -1 and b"debug_iql_eval_out" in err() and picked[0] == 0 and picked[1] == 0, what
    for bad, what in (((None, p, 4), "null dst"), ((p, None, 4), "null src"), ((p, p, 0), "n 0"), ((p, p, -5), "n < 0")):
        picked[0] = picked[1] = 7
        assert Cp(*bad, None, pk) == -1 and b"debug_iql_copy" in err() and picked[0] == 0 and picked[1] == 0, what

    # publish
    def pub(**kw):
        a = IL.PublishArgs()
        for n in a.q:
            for f in IL.NET_FIELDS:
                setattr(n, f, p)
            n.in_, n.out = 8, 1
        for f in ("W1T", "b1", "W2T", "b2", "W3", "b3", "W1F", "W2F"):
            setattr(a, f, (C.c_void_p * 2)(p, p))
        a.om = a.os = a.c_om = a.c_os = p
        a.S, a.SA, a.H, a.streams = 6, 8, 64, 1
        for k, v in kw.items():
            o = a
            *path, leaf = k.split("__")
            for q in path:
                o = getattr(o, q) if not q.isdigit() else o[int(q)]
            setattr(o, leaf, v)
        return a
    PB = "m3pc_debug_iql_publish"
    for H in (0, 32, 512):
        refused(PB, pub(H=H), b"hidden", f"hidden {H}")
    refused(PB, pub(S=0), b"S ", "S 0")
    refused(PB, pub(SA=6), b"S ", "no action")
    refused(PB, pub(SA=65), b"S ", "S + A 65")
    refused(PB, pub(S=30, SA=33, q__0__in_=33, q__1__in_=33), b"streams", "streams beyond 32 features")
    for f in ("om", "os", "c_om", "c_os", "q__1__W2", "q__0__b3"):
        refused(PB, pub(**{f: None}), b"null pointer", f)
    for f in ("W1T", "b1", "W2T", "b2", "W3", "b3", "W1F", "W2F"):
        refused(PB, pub(**{f: (C.c_void_p * 2)(p, None)}), b"null pointer", f)
    refused(PB, pub(q__1__in_=7), b"a critic has", "in != SA")
    refused(PB, pub(q__0__out=2), b"a critic has", "out 2")
