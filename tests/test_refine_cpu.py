"""The CEM / MPPI refinement as C calls, without a GPU: m3pc_refit_resample / m3pc_refine_plan are declared in
include/m3pc_hip.h, exported by the library and bound by m3pc_amd/capi.py; m3pc_refine_args has the header's layout; the
additions did not move the ABI version; null and bad arguments are refused before any HIP call is made.  And the fp64
restatement the GPU tests compare against (tests/refine_ref.py) is itself pinned: on torch.mean / torch.std for equal weights,
and on the oracle's cem_guiding for the whole loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import refine_ref as R
from m3pc_amd import build, capi, synth
from oracle import mtm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m3pc_refit_resample", "m3pc_refine_plan")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library(build.build_library())


def _header():
    return open(os.path.join(ROOT, "include", "m3pc_hip.h")).read()


def test_both_symbols_are_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/m3pc_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert hasattr(capi.Handle, "refit_resample") and hasattr(capi.Handle, "refine_plan")
    for macro, value in (("M3PC_REFINE_CEM", capi.REFINE_CEM), ("M3PC_REFINE_MPPI", capi.REFINE_MPPI),
                         ("M3PC_REFINE_MAX_ITER", capi.REFINE_MAX_ITER)):
        assert int(re.search(r"#define %s (\d+)" % macro, code).group(1)) == value
    assert "m3pc_refine_plan" in re.search(r"/\* ABI history\..*?\*/", _header(), flags=re.S).group(0)


def test_abi_version_did_not_move(lib):
    assert lib.m3pc_abi_version() == 7 == capi.ABI_VERSION
    assert int(re.search(r"#define M3PC_ABI_VERSION (\d+)", _header()).group(1)) == 7


def test_refine_args_layout_matches_the_header():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct m3pc_refine_args \{(.*?)\} m3pc_refine_args;", code, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(unsigned int|int|float)\s+(.*)", decl.strip(), flags=re.S)
        if m:
            fields += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    assert [n for _, n in fields] == [n for n, _ in capi.RefineArgs._fields_]
    ctypes_of = {"int": C.c_int, "float": C.c_float, "unsigned int": C.c_uint}
    for i, ((ctype, n), (_, ct)) in enumerate(zip(fields, capi.RefineArgs._fields_)):
        assert ct is ctypes_of[ctype], n
        assert getattr(capi.RefineArgs, n).offset == 4 * i, n  # (4-byte fields only: the header's order IS the layout)
    assert C.sizeof(capi.RefineArgs) == 40


def test_null_and_bad_arguments_are_refused_without_a_gpu(lib):
    fake = C.create_string_buffer(64)  # stands in for a handle: the argument checks come before the handle is touched
    h = C.c_void_p(C.addressof(fake))
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    args = capi.PlanArgs(capi.MODE_RTG, capi.PREC_FP32, 4, 64, 0, 64, 0.6, 0.99, 3.0, 0, 0, None, 0, 0)
    ref = capi.RefineArgs(2, 16, capi.REFINE_CEM, 0.0, 0.1, 0.0, 0, 0, 0, 0)

    def plan(h_, a_, r_, states=p, actions=p, rewards=p, mean=p, std=p, cand=p):
        return lib.m3pc_refine_plan(h_, a_, r_, states, actions, rewards, None, None, mean, std, cand, None, None, None, None, None)

    a, r = C.byref(args), C.byref(ref)
    assert plan(None, a, r) == -1 and b"null" in lib.m3pc_last_error()
    assert plan(h, None, r) == -1 and b"null" in lib.m3pc_last_error()
    assert plan(h, a, None) == -1 and b"null" in lib.m3pc_last_error()
    for name in ("states", "actions", "rewards", "mean", "std", "cand"):
        assert plan(h, a, r, **{name: None}) == -1 and b"null" in lib.m3pc_last_error(), name

    def bad(what, **kw):
        a2 = capi.PlanArgs.from_buffer_copy(args)
        r2 = capi.RefineArgs.from_buffer_copy(ref)
        for k, v in kw.items():
            setattr(a2 if hasattr(a2, k) else r2, k, v)
        assert plan(h, C.byref(a2), C.byref(r2)) == -1, kw
        msg = lib.m3pc_last_error()
        assert what in msg, (kw, msg)

    bad(b"one rank", n_count=32)
    bad(b"one rank", n_begin=1, n_count=63)
    bad(b"n_total", n_total=20000, n_count=20000)
    bad(b"precision", precision=5)
    bad(b"slot", slot=4)
    bad(b"mode", mode=capi.MODE_NOISE)
    bad(b"horizon", horizon=0)
    bad(b"flags", flags=capi.PLAN_DEFER_JOIN)
    bad(b"flags", flags=capi.PLAN_PRUNED_POLICY | 64)
    bad(b"iterations", iterations=0)
    bad(b"iterations", iterations=17)
    bad(b"top_k", top_k=0)
    bad(b"top_k", top_k=65)  # > n_total
    bad(b"weighting", weighting=2)
    bad(b"weighting", weighting=-1)
    bad(b"temperature", weighting=capi.REFINE_MPPI, temperature=-1.0)
    bad(b"temperature", weighting=capi.REFINE_MPPI, temperature=float("nan"))
    bad(b"temperature", weighting=capi.REFINE_MPPI, temperature=float("inf"))
    bad(b"init_std", init_std=-0.1)
    bad(b"init_std", init_std=float("nan"))
    bad(b"min_std", min_std=-1e-3)
    bad(b"min_std", min_std=float("inf"))

    # m3pc_refit_resample(h, cand, n, horizon, scores, elites, k, weighting, temperature, min_std, noise, mean, std, cand_out, stream)
    def refit(h_=h, cand=p, n=64, horizon=4, scores=p, elites=p, k=16, weighting=capi.REFINE_CEM, temperature=0.0, min_std=0.0,
              noise=None, mean=p, std=p, cand_out=None):
        return lib.m3pc_refit_resample(h_, cand, n, horizon, scores, elites, k, weighting, temperature, min_std, noise, mean, std, cand_out,
                                       None)

    for kw in (dict(h_=None), dict(cand=None), dict(elites=None), dict(mean=None), dict(std=None)):
        assert refit(**kw) == -1 and b"null" in lib.m3pc_last_error(), kw
    for what, kw in ((b"n ", dict(n=0)), (b"n ", dict(n=16385, k=1)), (b"k ", dict(k=0)), (b"k ", dict(k=65)), (b"horizon", dict(horizon=0)),
                     (b"weighting", dict(weighting=3)), (b"temperature", dict(weighting=capi.REFINE_MPPI, temperature=-0.5)),
                     (b"min_std", dict(min_std=float("nan"))), (b"scores", dict(weighting=capi.REFINE_MPPI, scores=None)),
                     (b"noise", dict(noise=p)), (b"noise", dict(cand_out=p))):
        assert refit(**kw) == -1, kw
        assert what in lib.m3pc_last_error(), (kw, lib.m3pc_last_error())


@pytest.mark.parametrize("k", [1, 2, 16, 65])
def test_reference_refit_with_equal_weights_is_torch_mean_and_std(k):
    rng = np.random.RandomState(k)
    cand = rng.uniform(-1, 1, size=(130, 4, 3))
    elites = rng.permutation(130)[:k]
    mean, std, D = R.refit(cand, elites)
    el = torch.from_numpy(cand)[torch.from_numpy(elites)]
    assert np.abs(mean - el.mean(dim=0).numpy()).max() <= 1e-12
    exp_std = el.std(dim=0).numpy() if k > 1 else np.zeros((4, 3))
    assert np.abs(std - exp_std).max() <= 1e-12
    assert abs(D - (1.0 - 1.0 / k)) <= 1e-12
    # the floor, and MPPI at temperature 0 is the same estimate
    assert np.array_equal(R.refit(cand, elites, min_std=2.0)[1], np.full((4, 3), 2.0))
    m2, s2, _ = R.refit(cand, elites, rng.normal(size=130), R.MPPI, 0.0)
    assert np.abs(m2 - mean).max() <= 1e-12 and np.abs(s2 - std).max() <= 1e-12


def test_reference_weights_and_resample():
    w = R.weights([3.0, 1.0, 3.0], R.MPPI, 0.5)
    assert abs(w.sum() - 1.0) <= 1e-15 and w[0] == w[2] and abs(w[1] / w[0] - np.exp(-1.0)) <= 1e-15
    assert np.array_equal(R.weights([0.0, 1.0, 5.0], R.MPPI, 1e4), [0.0, 0.0, 1.0])  # one-hot: D = 0, std = 0
    assert R.refit(np.arange(6.0).reshape(3, 2, 1), [0, 1, 2], [0.0, 1.0, 5.0], R.MPPI, 1e4)[2] == 0.0
    assert np.array_equal(R.top_k(np.array([1.0, 3.0, 3.0, 0.0, 3.0]), 3), [1, 2, 4])  # ties to the lower index
    mean, std = np.float32([[0.5, -0.9]]), np.float32([[0.25, 0.5]])
    noise = np.float32([[[4.0, -1.0]], [[-8.0, 0.1]]])
    out = R.resample(mean, std, noise)
    assert out.dtype == np.float32 and np.array_equal(out, np.float32([[[1.0, -1.0]], [[-1.0, np.float32(-0.9) + np.float32(0.5) * np.float32(0.1)]]]))


@pytest.mark.parametrize("mode,N,k", [("rtg", 130, 65), ("critic", 64, 16)])
def test_reference_loop_reproduces_the_oracle_cem_trace(mode, N, k):
    """refine_ref against oracle.cem_guiding on the tiny config, with oracle.plan_candidates as the scorer.
    Link by link on the oracle's own trace, everything that can be exact is: the candidates resampled from the oracle's
    distribution of iteration `it` are the oracle's bits, so their scores are the oracle's scores bit for bit, and top_k gives the
    oracle's elite list.  The refit cannot be bit-equal -- the oracle refits in fp32 (torch.mean / torch.std over k rows), the
    restatement in fp64 -- and agrees to the rounding of a k-term fp32 sum of values in [-1, 1], 2 k 2^-24.
    The free-running loop then carries those refit differences forward: its candidates differ from the oracle's by that bound times
    (1 + |noise|) plus one fp32 rounding; its elite lists must still be the oracle's lists (both cases have a clear elite boundary),
    and its distributions stay within the same refit bound of the oracle's next ones."""
    dims = synth.Dims(11, 3, 8, n_embd=64, n_head=2)
    sd, st = synth.make_state_dict(dims, 0), O.make_stats(synth.make_tokenizer_stats(dims, 0))
    critic = synth.make_critic(dims, 0)
    hist = synth.make_history(dims, 0)
    ocfg = O.PlanCfg(8, 4, N, n_head=2)
    win, h = O.assemble_window(ocfg, hist, 100, 3.0)
    noise = torch.randn(3, N, h, 3, generator=torch.Generator().manual_seed(11))
    lmbda = 0.6
    ref = O.cem_guiding(sd, st, ocfg, win, h, lmbda, noise, mode, critic=critic, iterations=2, top_k=k)
    loc, _ = O.policy_pass(sd, st, ocfg, win, h)
    mean0 = torch.tanh(loc[0, 8 - h:, 0, :]).numpy()

    def score(cand):
        return O.plan_candidates(sd, st, ocfg, win, h, torch.from_numpy(cand), mode, lmbda, critic).numpy()

    tol = 2 * k * 2.0 ** -24
    # link by link on the oracle's trace
    mean, std = mean0, np.full_like(mean0, np.float32(0.1))
    for it, e in enumerate(ref["trace"]):
        cand = R.resample(mean, std, noise[it].numpy())
        er = score(cand)
        assert np.array_equal(er, e["expect_return"].numpy())
        top = R.top_k(er, k)
        assert top.tolist() == e["top"].tolist()
        m64, s64, _ = R.refit(cand, top)
        assert np.abs(m64 - e["mean"].numpy()).max() <= tol and np.abs(s64 - e["std"].numpy()).max() <= tol
        mean, std = e["mean"].numpy(), e["std"].numpy()
    assert np.array_equal(R.resample(mean, std, noise[2].numpy()), ref["candidates"].numpy())
    # the free-running loop
    got = R.loop(score, mean0, 0.1, noise.numpy(), 2, k)
    ctol = tol * (1.0 + float(noise.abs().max())) + 2.0 ** -23  # (mean + std * z from distributions tol apart, then rounded)
    for it in range(2):
        g, e = got["trace"][it], ref["trace"][it]
        assert g["top"].tolist() == e["top"].tolist()
        # (iteration 1 refits candidates that are ctol apart on the same elites: a weighted mean / spread moves by no more)
        lim = tol if it == 0 else tol + 2 * ctol
        assert np.abs(g["mean"] - e["mean"].numpy()).max() <= lim and np.abs(g["std"] - e["std"].numpy()).max() <= lim
    assert np.array_equal(got["trace"][0]["expect_return"], ref["trace"][0]["expect_return"].numpy())  # (same first candidates)
    lim = tol + 2 * ctol
    assert np.abs(got["candidates"] - ref["candidates"].numpy()).max() <= lim * (1.0 + float(noise.abs().max())) + 2.0 ** -23
    assert np.abs(got["eval_action"] - ref["eval_action"].numpy()).max() <= lim
    assert np.array_equal(got["mean"][0], mean0) and np.all(got["std"][0] == np.float32(0.1))
