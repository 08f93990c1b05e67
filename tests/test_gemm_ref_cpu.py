"""CPU checks of tests/gemm_ref.py, the float64 GEMM reference and bound the GPU test (test_gemm_edges_gpu.py) holds every GEMM kernel
to: the reference is torch's own linear / gelu / layer_norm in float64; plain fp32 restatements of the kernels' arithmetic stay
inside the bound in every input regime (so an honest kernel can meet it) and equal the reference in the `int` regime; and every
seeded bug breaks the `int` equality and, where the bound can see it, the bound."""
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as R


def _phys(t, M, amap, cmap, seed, integer):
    """Physical A and res tensors of a row-mapped case: the logical rows at their mapped places, other values in the gaps."""
    g = torch.Generator().manual_seed(seed)
    junk = (lambda *s: torch.randint(-3, 4, s, generator=g).float()) if integer else (lambda *s: torch.randn(*s, generator=g))
    arow, crow = R.map_rows(amap, M), R.map_rows(cmap, M)
    A = junk(int(arow.max()) + 3, t["A"].shape[1])
    A[arow] = t["A"]
    res = None
    if t["res"] is not None:
        res = junk(int(crow.max()) + 3, t["res"].shape[1])
        res[crow] = t["res"]
    return A, res


def _ln32(x, g, b, unbiased=False):
    if unbiased:
        return R.layernorm64(x, g, b, unbiased=True).float()
    return F.layer_norm(x.float(), x.shape[-1:], g.float(), b.float(), 1e-5)


def kernel_like(P, dtype, f32out=True, loop=False, bug=None):
    """fp32 restatement of what a kernel computes for problem P (the arguments of gemm_ref), with optional seeded bugs."""
    M, amap = P["M"], P["amap"]
    if bug == "amap_no_off":
        amap = (amap[0], amap[1], 0)
    arow, crow = R.map_rows(amap, M), R.map_rows(P["cmap"], M)
    a, w = P["A"][arow].float().clone(), P["W"].float()
    if P["a_ln"] is not None:
        a = _ln32(a, *P["a_ln"], unbiased=bug == "a_ln_unbiased")
    extra = None
    if bug is not None and bug[0] == "drop":
        a[:, bug[1]:bug[1] + bug[2]] = 0
    if bug is not None and bug[0] == "dup":
        extra = a[:, bug[1]:bug[1] + bug[2]] @ w[:, bug[1]:bug[1] + bug[2]].T

    def product(a, w):
        if not loop:
            return a @ w.T
        acc = torch.zeros(a.shape[0], w.shape[0])
        for k in reversed(range(a.shape[1])):  # (one fp32 fma per k, last k first)
            acc = acc + a[:, k:k + 1] * w[:, k].unsqueeze(0)
        return acc
    if dtype == 2:
        ah, wh = a.bfloat16().float(), w.bfloat16().float()
        al, wl = (a - ah).bfloat16().float(), (w - wh).bfloat16().float()
        v = product(ah, wh) + product(ah, wl) + product(al, wh)
    else:
        v = product(a, w)
    if extra is not None:
        v = v + extra
    if P["bias"] is not None and bug != "no_bias":
        v = v + P["bias"].float()
    if P["rowtab"] is not None:
        mod = P["rt_mod"] + (1 if bug == "rt_mod+1" else -1 if bug == "rt_mod-1" else 0)
        tab = torch.cat([P["rowtab"].float(), P["rowtab"].float()[:1] + 1])  # (the row a too large modulus reads behind the table)
        v = v + tab[torch.arange(M) % mod]
    gelu = (lambda x: R.gelu_fast_f64(x)) if dtype == 1 else (lambda x: F.gelu(x))
    if P["gelu"] and bug != "gelu_after_res":
        v = gelu(v)
    if P["res"] is not None:
        v = v + P["res"].float()[torch.arange(M) if bug == "res_unmapped" else crow]
    if P["gelu"] and bug == "gelu_after_res":
        v = gelu(v)
    if bug == "swap_cols":
        v = torch.cat([v[:, 64:128], v[:, :64], v[:, 128:]], 1)
    if bug == "shift_row":
        v = torch.roll(v, 1, 0)
    assert v.dtype == torch.float32
    return v if f32out else v.bfloat16().float()


def problem(regime, dtype, M=96, N=128, K=256, bias=True, rt_mod=8, res=True, gelu=False, maps=True, a_ln=False, ln=False, seed=0,
            spike_k=None):
    t = R.make_inputs(regime, M, N, K, dtype=dtype, bias=bias, rt_mod=rt_mod, res=res, spike_k=spike_k, seed=seed)
    amap, cmap = ((8, 32, 8), (8, 32, 16)) if maps else (None, None)
    A, resp = _phys(t, M, amap, cmap, seed + 1, regime == "int")
    g = torch.Generator().manual_seed(seed + 2)
    lnp = lambda d: (1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g))
    return dict(A=A, W=t["W"], M=M, bias=t["bias"], rowtab=t["rowtab"], rt_mod=max(rt_mod, 1), gelu=gelu, res=resp, amap=amap,
                cmap=cmap, a_ln=lnp(K) if a_ln else None, ln=lnp(N) if ln else None)


def ratio(P, dtype, got, f32out=True, S_split=1):
    ref = R.gemm_ref(**P)
    bnd = R.bound(ref, dtype, P["A"].shape[1], S_split, f32out)
    return float(((got.double() - ref["C"]).abs() / bnd).max()), ref


def test_reference_is_torch_in_float64():
    g = torch.Generator().manual_seed(0)
    M, N, K = 37, 64, 96
    A, W, b = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((M, K), (N, K), (N,)))
    res, rt = torch.randn(M, N, generator=g, dtype=torch.float64), torch.randn(5, N, generator=g, dtype=torch.float64)
    gk, bk, gn, bn = (torch.randn(d, generator=g, dtype=torch.float64) for d in (K, K, N, N))
    ref = R.gemm_ref(A, W, bias=b, gelu=True, res=res)
    assert torch.allclose(ref["C"], F.gelu(F.linear(A, W, b)) + res, rtol=0, atol=1e-13)
    assert torch.allclose(ref["S"], A.abs() @ W.abs().T, rtol=0, atol=1e-12)
    ref = R.gemm_ref(A, W, rowtab=rt, rt_mod=5, a_ln=(gk, bk), ln=(gn, bn))
    want = F.linear(F.layer_norm(A, (K,), gk, bk, 1e-5), W) + rt[torch.arange(M) % 5]
    assert torch.allclose(ref["C"], want, rtol=0, atol=1e-12)
    assert torch.allclose(ref["ln"](want), F.layer_norm(want, (N,), gn, bn, 1e-5), rtol=0, atol=1e-12)
    # row maps: logical row r of A and of C / res at (r / rpg) gstride + r % rpg + off
    Ap, resp = torch.randn(64, K, generator=g, dtype=torch.float64), torch.randn(64, N, generator=g, dtype=torch.float64)
    ref = R.gemm_ref(Ap, W, M=12, res=resp, amap=(4, 16, 4), cmap=(4, 16, 8))
    rows_a = torch.tensor([4, 5, 6, 7, 20, 21, 22, 23, 36, 37, 38, 39])
    assert torch.equal(ref["crow"], rows_a + 4)
    assert torch.allclose(ref["C"], F.linear(Ap[rows_a], W) + resp[rows_a + 4], rtol=0, atol=1e-12)


def test_gelu_fast_formula_error():
    """The Abramowitz-Stegun formula of gelu_fast, in float64 on a dense grid, is within its stated 1.5e-7 on erf (|x| / 2 of it on
    the GELU): the measured value is what the module docstring of gemm_ref quotes."""
    x = R.gelu_grid()
    d = (R.gelu_fast_f64(x) - R.gelu64(x)).abs()
    erf_err = float((d[x != 0] / (0.5 * x[x != 0].abs())).max())
    print(f"gelu_fast formula: max error on erf {erf_err:.3g} (stated {R.AS_ERR:.3g}), on the GELU {float(d.max()):.3g}")
    assert erf_err <= R.AS_ERR
    xs = torch.linspace(-4, 4, 80001, dtype=torch.float64)
    eps = 1e-6
    assert float(((R.gelu64(xs + eps) - R.gelu64(xs - eps)) / (2 * eps)).abs().max()) <= R.GELU_LIP


@pytest.mark.parametrize("regime", R.REGIMES)
def test_fp32_restatements_stay_inside_the_bound(regime):
    """torch's fp32 matmul, a sequential fp32 fma loop from the last k to the first, and the bf16-rounded output, for every operand
    type and epilogue: all inside the bound; in the `int` regime without GELU they equal the reference."""
    worst = 0.0
    for dtype in (0, 1, 2):
        for ci, (gelu, res, rt_mod, maps, a_ln, K) in enumerate([(False, True, 8, True, False, 256), (True, False, 0, False, False, 512),
                                                                 (False, False, 8, True, False, 2048), (False, True, 0, False, dtype == 0, 512)]):
            if a_ln and regime == "int":
                continue
            for spike_k in ((31, 32, K - 1) if regime == "spike" else (None,)):
                P = problem(regime, dtype, M=40, N=128, K=K, res=res, rt_mod=rt_mod, gelu=gelu, maps=maps, a_ln=a_ln, seed=10 * ci + dtype,
                            spike_k=spike_k)
                for loop in (False, True) if K <= 512 else (False,):
                    for f32out in (True, False) if dtype else (True,):
                        got = kernel_like(P, dtype, f32out=f32out, loop=loop)
                        r, ref = ratio(P, dtype, got, f32out)
                        assert r <= 1.0, (regime, dtype, ci, loop, f32out, r)
                        worst = max(worst, r)
                        if regime == "int" and not gelu:
                            want = ref["C"] if f32out else ref["C"].float().bfloat16().double()
                            assert torch.equal(got.double(), want), (dtype, ci, loop, f32out)
                        if regime == "spike":
                            k = P["A"].shape[1] - 1 if spike_k is None else spike_k
                            a = P["A"][R.map_rows(P["amap"], P["M"])].double()
                            share = (a[:, k].abs().unsqueeze(1) * P["W"][:, k].double().abs().unsqueeze(0)) / ref["S"]
                            assert float(share.median()) > 0.5, "spike regime: the spiked k does not carry most of S"
                        if regime == "offset":
                            assert float((ref["acc"].abs() / ref["S"]).median()) < 0.05
    print(f"fp32 restatement, regime {regime}: largest err / bound {worst:.3g}")


def test_layernorm_bound_holds_for_fp32_layernorm():
    for regime in ("randn", "offset", "int"):
        P = problem(regime, 0, M=64, N=512, K=256, ln=True, maps=False, seed=5)
        C = kernel_like(P, 0)
        ref = R.gemm_ref(**P)
        y = _ln32(C, *P["ln"])
        r = float(((y.double() - ref["ln"](C)).abs() / R.ln_bound(C, *P["ln"])).max())
        print(f"fp32 LayerNorm of C, regime {regime}: largest err / bound {r:.3g}")
        assert r <= 1.0
        yb = _ln32(C, *P["ln"], unbiased=True)
        assert float(((yb.double() - ref["ln"](C)).abs() / R.ln_bound(C, *P["ln"])).max()) > 1.0, "unbiased variance passes"


# (bug, seen by the bound in randn or spike as well)
BUGS = [(("drop", 64, 16), True), (("drop", 32, 32), True), (("drop", 192, 64), True), (("dup", 128, 32), True), (("drop", 77, 1), False),
        ("swap_cols", True), ("shift_row", True), ("no_bias", True), ("rt_mod+1", True), ("rt_mod-1", True), ("res_unmapped", True),
        ("gelu_after_res", True), ("amap_no_off", True), ("a_ln_unbiased", True)]


@pytest.mark.parametrize("bug,dagger", BUGS, ids=[b if isinstance(b, str) else "%s_%d_%d" % b for b, _ in BUGS])
def test_seeded_bug_is_caught(bug, dagger):
    """Each bug breaks the `int` equality (with a GELU or a LayerNorm in the problem nothing is exact: the bound there), each one
    marked also exceeds the bound in randn or spike -- for fp32 output of bf16 and of fp32 operands."""
    gelu, a_ln = bug == "gelu_after_res", bug == "a_ln_unbiased"
    for dtype in (0,) if a_ln else (0, 1):
        if not a_ln:
            P = problem("int", dtype, gelu=gelu, seed=3)
            assert torch.equal(kernel_like(P, dtype).double(), R.gemm_ref(**P)["C"]) or gelu
            got = kernel_like(P, dtype, bug=bug)
            if gelu:
                assert ratio(P, dtype, got)[0] > 1.0
            else:
                assert not torch.equal(got.double(), R.gemm_ref(**P)["C"]), f"{bug}: the int regime does not see it"
        if dagger:
            seen = []
            for regime in ("randn", "spike"):
                P = problem(regime, dtype, gelu=gelu, a_ln=a_ln, K=512 if a_ln else 256, seed=4, spike_k=bug[1] if not isinstance(bug, str) else None)
                assert ratio(P, dtype, kernel_like(P, dtype))[0] <= 1.0
                seen.append(ratio(P, dtype, kernel_like(P, dtype, bug=bug))[0])
            assert max(seen) > 1.0, f"{bug}: err / bound {seen} in randn / spike"


def test_case_table_names_what_the_dispatch_picks():
    """The GPU test's case table against the lab library's plan-only entry (the checks and the walk of the dispatch of
    m3pc_debug_gemm_ex, nothing launched): every case is accepted and reaches the kernel id, split count, peel row and flags it names,
    and every refusal of the GPU test is a refusal -- without a GPU."""
    import ctypes as C

    import test_gemm_edges_gpu as E
    lib = E.lab()
    for c in E.CASES:
        rc, planned = E.plan_of(lib, c)
        assert rc == 0, (c["name"], lib.m3pc_last_error())
        assert planned == c["expect"], (c["name"], planned, c["expect"])
    for what, c, edit in E.refusal_cases():
        picked = (C.c_int * 4)()
        a = E.edit_args(E.fill_args(c, E.layout(c), lambda name: 0x10000000, picked), edit)
        assert lib.m3pc_debug_gemm_plan(C.byref(a)) != 0, what
        assert tuple(picked) == (0, 0, 0, 0) and lib.m3pc_last_error(), what
    assert E.header_ids() == set(range(1, 14))
