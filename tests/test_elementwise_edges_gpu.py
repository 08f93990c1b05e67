"""Every kernel of m3pc_amd/csrc/elementwise.hip at its row and lane edges, each alone through its lab hook (include/m3pc_hip_debug.h:
m3pc_debug_layernorm, _head_out, _actor_head, _critic, _sample, _score, _gather_rows, _goal_overlay, _goal_overlay_rows, _embed; the
tokeniser through m3pc_tokenize / m3pc_detokenize) against the references of tests/elementwise_ref.py.

Each case names the kernel id its launch must report (`picked`; the list is in the header, "Elementwise kernel ids");
test_every_elementwise_kernel_has_a_case checks that the cases reach exactly the ids of that list.  Where a kernel has arithmetic a
case runs in three regimes: `int` must EQUAL the reference (small integers and powers of two: any summation order and the hi / lo split
are exact), `randn` and `offset` (|mean| >> sd) are held to the derived element-wise bound.  The kernels without arithmetic of their
own order (sample, score, gather_rows, tokeniser, overlays) are held bit for bit to a float32 restatement.  Everything a kernel may not
read holds NaN (padding columns of a padded ldx, rows a row map skips, weight rows >= A or >= D, a bf16 copy the dispatch must not take);
every output buffer holds a sentinel in its padding and in a guard row and is compared bit for bit with its state before the call
outside the elements the call owns."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import elementwise_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -31744.0  # exact in bf16 and fp32; no case comes near it
DEV = "cuda"
vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
pi = C.POINTER(ci)
REGIMES = ("int", "randn", "offset")
WORST = {}     # (kernel id, output) -> largest err / bound of the randn and offset regimes
EXACT = {}     # kernel id -> int-regime and bit-for-bit comparisons that were exact
REACHED = set()


class LnArgs(C.Structure):
    _fields_ = [("X", vp), ("ldx", ci), ("xmap", ci * 3), ("rows", ci), ("d", ci), ("g1", vp), ("b1", vp), ("g2", vp), ("b2", vp),
                ("Yf", vp), ("Yb", vp), ("stream", vp), ("picked", pi)]


class HeadArgs(C.Structure):
    _fields_ = [("X", vp), ("Xb", vp), ("ldx", ci), ("rows", ci), ("d", ci), ("D", ci), ("W", vp), ("b", vp), ("mean", vp), ("stdv", vp),
                ("Y", vp), ("ymap", ci * 3), ("ldy", ci), ("stream", vp), ("picked", pi)]


class ActorArgs(C.Structure):
    _fields_ = [("X", vp), ("ldx", ci), ("xmap", ci * 3), ("rows", ci), ("d", ci), ("A", ci), ("Wmu", vp), ("bmu", vp), ("Wls", vp),
                ("bls", vp), ("mu", vp), ("sd", vp), ("ln_g", vp), ("ln_b", vp), ("stream", vp), ("picked", pi)]


class CriticArgs(C.Structure):
    _fields_ = [("states", vp), ("actions", vp), ("rows", ci), ("S", ci), ("A", ci), ("hidden", ci), ("om", vp), ("os", vp), ("W1", vp * 2),
                ("b1", vp * 2), ("W2", vp * 2), ("b2", vp * 2), ("W3", vp * 2), ("b3", vp * 2), ("q", vp), ("force_scalar", ci), ("stream", vp),
                ("picked", pi)]


class SampleArgs(C.Structure):
    _fields_ = [("hist_actions", vp), ("loc", vp), ("sd", vp), ("eps", vp), ("mode", ci), ("T", ci), ("A", ci), ("idx", ci), ("h", ci),
                ("n_begin", ci), ("n_count", ci), ("widx", vp), ("index", vp), ("cand", vp), ("sample_actions", vp), ("loc_out", vp),
                ("sd_out", vp), ("eps_rows", ll), ("hist_windows", ci), ("stream", vp), ("picked", pi)]


class ScoreArgs(C.Structure):
    _fields_ = [("rewards", vp), ("boot", vp), ("n", ci), ("h", ci), ("boot_scale", C.c_float), ("gamma", C.c_float), ("lmbda", C.c_double),
                ("expect_return", vp), ("boot_out", vp), ("scatter_index", vp), ("scatter_out", vp), ("stream", vp), ("picked", pi)]


class GatherArgs(C.Structure):
    _fields_ = [("Xe", vp), ("xe_bstride", ll), ("table", vp), ("rowsrc", vp), ("rows_per_batch", ci), ("batch", ci), ("d", ci), ("out", vp),
                ("outb", vp), ("xe_rows", ci), ("table_rows", ci), ("stream", vp), ("picked", pi)]


class EmbedArgs(C.Structure):
    """m3pc_debug_embed_args."""
    _fields_ = [("tok", vp * 4), ("bstride", ll * 4), ("WT", vp * 4), ("E", vp * 4), ("feat", ci * 4), ("tokmap", vp), ("batch", ci),
                ("L", ci), ("d", ci), ("T", ci), ("X", vp), ("Xb", vp), ("ln_g", vp), ("ln_b", vp), ("Hb", vp), ("Hb_sh", vp),
                ("n_indep", ci), ("n_sh", ci), ("x_first_only", ci), ("x_compact", ci), ("stream", vp)]


class EmbedExArgs(C.Structure):
    """m3pc_debug_embed_ex_args."""
    _fields_ = [("base", EmbedArgs), ("Hf", vp), ("picked", pi)]


HOOKS = {"m3pc_debug_embed_ex": EmbedExArgs, "m3pc_debug_layernorm": LnArgs, "m3pc_debug_head_out": HeadArgs, "m3pc_debug_actor_head": ActorArgs, "m3pc_debug_critic": CriticArgs,
         "m3pc_debug_sample": SampleArgs, "m3pc_debug_score": ScoreArgs, "m3pc_debug_gather_rows": GatherArgs, "m3pc_debug_embed": EmbedArgs}


def lab():
    from hip_util import lab_library
    lib = lab_library()
    for name, st in HOOKS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ci, [C.POINTER(st)]
    fp = C.POINTER(C.c_float)
    lib.m3pc_debug_critic_pack.restype, lib.m3pc_debug_critic_pack.argtypes = ci, [fp, fp, ci, ci, fp, fp, C.POINTER(ll), C.POINTER(ll)]
    lib.m3pc_debug_goal_overlay.restype, lib.m3pc_debug_goal_overlay.argtypes = ci, [vp, vp, vp, ll, ci, ci, ci, vp, vp, ci, vp, pi]
    lib.m3pc_debug_goal_overlay_rows.restype, lib.m3pc_debug_goal_overlay_rows.argtypes = ci, [vp, vp, vp, ll, ci, ci, ci, ci, vp, pi]
    lib.m3pc_debug_elementwise_picked.restype, lib.m3pc_debug_elementwise_picked.argtypes = ci, []
    return lib


def header_ids():
    src = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    block = src[src.index("Elementwise kernel ids"):src.index("(not listed, no id")]
    return {int(n): k for n, k in re.findall(r"(?:^|;|\*)\s*(\d+) ([a-z0-9_]+_kernel(?:<[0-9, ]+>)?)", block, re.M)}


@pytest.fixture(scope="module")
def lib():
    return lab()


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def call(lib, fn, a, want, what):
    """Runs a hook, checks its return code and the kernel id it reports."""
    picked = (ci * 1)(-1)
    a.picked = C.cast(picked, pi)
    a.stream = stream()
    rc = getattr(lib, fn)(C.byref(a))
    assert rc == 0, (what, lib.m3pc_last_error())
    torch.cuda.synchronize()
    assert picked[0] == want, f"{what}: the launcher reports kernel {picked[0]}, the case is for {want}"
    REACHED.add(want)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def nan_rows(x, ld, prow=None, et=torch.float32):
    """x's rows at physical rows prow (default: in order) of a NaN buffer with leading dimension ld and a NaN row behind."""
    prow = torch.arange(x.shape[0], device=DEV) if prow is None else prow
    buf = torch.full((int(prow.max()) + 2, ld), float("nan"), device=DEV, dtype=et)
    buf[prow, :x.shape[1]] = x.to(et)
    return buf


def sent(rows, ld, et=torch.float32):
    return torch.full((rows + 1, ld), SENT, device=DEV, dtype=et)


def owned(buf, before, rows, ncols, what):
    """The elements the call owns, all written; outside them the buffer has the bits it had before the call."""
    after = buf.clone()
    after[rows, :ncols] = before[rows, :ncols]
    assert torch.equal(_bits(after), _bits(before)), f"{what}: a padding column, a guard row or a row of no owner was written"
    o = buf[rows, :ncols]
    assert not bool((o == SENT).any()), f"{what}: an element was not written"
    return o


def same(t, before, what):
    assert torch.equal(_bits(t), _bits(before)), f"{what}: an input was written"


def hold(kid, key, out, ref, bound, regime, what):
    """int: equality; randn / offset: err <= bound, the ratio recorded."""
    out = out.double()
    assert bool(torch.isfinite(out).all()), f"{what}: {key} is not finite"
    if regime == "int":
        assert torch.equal(out, ref), f"{what}: {key} differs from the exact result at {int((out != ref).sum())} elements, largest {float((out - ref).abs().max())}"
        EXACT[kid] = EXACT.get(kid, 0) + 1
        return
    ratio = float(((out - ref).abs() / bound).max())
    WORST[(kid, key)] = max(WORST.get((kid, key), 0.0), ratio)
    assert ratio <= 1, f"{what}: {key} err / bound {ratio:.3g}"


def exact(kid, got, want, what):
    """Bit for bit against a float32 numpy restatement."""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the float32 restatement"
    EXACT[kid] = EXACT.get(kid, 0) + 1


MAP = (3, 5, 2)  # {rpg, gstride, off}: rows in groups of 3, the groups 5 rows apart, 2 rows in


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_D = (64, 192, 256, 512, 768, 1024)
LN_ROWS = (1, 3, 4, 5, 8191, 8192, 8193, 8199)


def ln_kernel(d, ldx, rows):
    """launch_layernorm's dispatch, restated."""
    if d % 256 or ldx % 4:
        return 7
    return 8 + d // 256 if rows >= 8192 else 8


def _ln_cases():
    cs = []
    for di, d in enumerate(LN_D):
        for ri, rows in enumerate(LN_ROWS):
            k = di * len(LN_ROWS) + ri
            pad = (0, 4, 1 if d % 256 == 0 else 4)[(di + ri) % 3]
            cs.append(dict(d=d, rows=rows, ldx=d + pad, mapped=bool((k // 2) % 2), double=bool((di + ri // 2) % 2), outs=("f", "b", "fb")[k % 3]))
    # the many-row kernel with everything at once, at an odd row count (its second row clamps to rows - 1), and the named pair
    cs += [dict(d=512, rows=8193, ldx=516, mapped=True, double=True, outs="fb"), dict(d=256, rows=8199, ldx=256, mapped=True, double=False, outs="b"),
           dict(d=1024, rows=8193, ldx=1024, mapped=False, double=True, outs="f"), dict(d=768, rows=8193, ldx=772, mapped=True, double=True, outs="fb"),
           dict(d=512, rows=8192, ldx=512, mapped=False, double=False, outs="fb", want=10), dict(d=512, rows=8191, ldx=512, mapped=False, double=False, outs="fb", want=8),
           dict(d=512, rows=8192, ldx=513, mapped=False, double=True, outs="fb", want=7)]
    for c in cs:
        c["name"] = f"ln_d{c['d']}_r{c['rows']}_ld{c['ldx']}" + ("_map" if c["mapped"] else "") + ("_double" if c["double"] else "") + "_Y" + c["outs"]
        c["kid"] = ln_kernel(c["d"], c["ldx"], c["rows"])
        assert c.get("want", c["kid"]) == c["kid"]
    return list({c["name"]: c for c in cs}.values())


LN_CASES = _ln_cases()


def ln_launch(lib, c, X, g1, b1, g2, b2, outs, what):
    rows, d = c["rows"], c["d"]
    a = LnArgs()
    a.X, a.ldx, a.rows, a.d = P(X), c["ldx"], rows, d
    a.xmap = (ci * 3)(*(MAP if c["mapped"] else (0, 0, 0)))
    a.g1, a.b1, a.g2, a.b2 = P(g1), P(b1), P(g2), P(b2)
    Yf = sent(rows, d) if "f" in outs else None
    Yb = sent(rows, d, torch.bfloat16) if "b" in outs else None
    bf, bb = (None if Yf is None else Yf.clone()), (None if Yb is None else Yb.clone())
    a.Yf, a.Yb = P(Yf), P(Yb)
    Xbefore = X.clone()
    call(lib, "m3pc_debug_layernorm", a, c["kid"], what)
    same(X, Xbefore, what)
    r = torch.arange(rows, device=DEV)
    return (None if Yf is None else owned(Yf, bf, r, d, what + " Yf")), (None if Yb is None else owned(Yb, bb, r, d, what + " Yb"))


@pytest.mark.parametrize("c", LN_CASES, ids=[c["name"] for c in LN_CASES])
def test_layernorm_against_float64(lib, c):
    rows, d, kid = c["rows"], c["d"], c["kid"]
    prow = R.map_rows(MAP if c["mapped"] else None, rows, DEV)
    for ri, regime in enumerate(REGIMES):
        what = f"{c['name']}/{regime}"
        x, g1, b1, g2, b2 = R.ln_inputs(regime, rows, d, c["double"], DEV, 100 * d + rows + ri)
        X = nan_rows(x, c["ldx"], prow)
        Yf, Yb = ln_launch(lib, c, X, g1, b1, g2, b2, c["outs"], what)
        norm = R.ln_int_ref if regime == "int" else R.layernorm64
        y1, B1 = norm(x, g1, b1), R.ln_bound(x, g1, b1)
        if c["double"]:
            if regime == "int":
                own1 = y1.float()
            else:  # the kernel's own first stage: the same launch without the second norm
                own1, _ = ln_launch(lib, c, X, g1, b1, None, None, "f", what + " (first stage)")
                hold(kid, "Y1", own1, y1, B1, regime, what)
            ref, B = norm(own1, g2, b2), R.ln_bound(own1, g2, b2)
        else:
            ref, B = y1, B1
        if Yf is not None:
            hold(kid, "Yf", Yf, ref, B, regime, what)
        if Yb is not None:
            hold(kid, "Yb", Yb.float(), ref, R.bf16_out_bound(ref, B), regime, what)
        if Yf is not None and Yb is not None:
            assert torch.equal(_bits(Yf.to(torch.bfloat16)), _bits(Yb)), f"{what}: Yb is not the bf16 rounding of Yf"


# ------------------------------------------------------------------------------------------------ head_out
def _head_cases():
    cs = []
    for di, d in enumerate((64, 512, 1024)):
        for Di, D in enumerate((1, 17, 32)):
            cs.append(dict(name=f"head_scalar_d{d}_D{D}", kid=13, d=d, D=D, rows=(1, 4, 5, 130), k=di + Di))
    for Di, D in enumerate((1, 4, 5, 17, 32)):
        cs.append(dict(name=f"head_mfma_D{D}", kid=14, d=512, D=D, rows=(2048, 2049, 2175), k=Di))
        cs.append(dict(name=f"head_mfma_D{D}_second_trip", kid=14, d=512, D=D, rows=(65537,), k=Di + 1))
    return cs


HEAD_CASES = _head_cases()


@pytest.mark.parametrize("c", HEAD_CASES, ids=[c["name"] for c in HEAD_CASES])
def test_head_out_against_float64(lib, c):
    d, D, kid = c["d"], c["D"], c["kid"]
    mfma = kid == 14
    for ri, rows in enumerate(c["rows"]):
        k = c["k"] + ri
        mapped, detok, pad = bool(k % 2), bool((k // 2) % 2) or rows == 65537, bool(k % 3 == 1)
        prow = R.map_rows(MAP if mapped else None, rows, DEV)
        ldx, ldy = d + ((8 if mfma else 1) if pad else 0), D + (3 if pad else 0)
        for gi, regime in enumerate(REGIMES):
            what = f"{c['name']}_r{rows}" + ("_map" if mapped else "") + ("_detok" if detok else "") + f"/{regime}"
            x, W, b, mean, stdv = R.head_inputs(regime, rows, d, D, DEV, 7 * rows + D + gi, bf16_rows=mfma)
            Wp = nan_rows(W, d)  # (a NaN weight row behind row D - 1)
            a = HeadArgs()
            if mfma:
                Xb = nan_rows(x, ldx, et=torch.bfloat16)
                a.Xb, src = P(Xb), Xb
            else:
                X = nan_rows(x, ldx)
                a.X, src = P(X), X
                if d == 512 and rows == 130:  # bf16 rows the dispatch must not take below 2048 rows
                    poison = torch.full((rows, ldx), float("nan"), device=DEV, dtype=torch.bfloat16)
                    a.Xb = P(poison)
            a.ldx, a.rows, a.d, a.D, a.W, a.b = ldx, rows, d, D, P(Wp), P(b)
            if detok:
                a.mean, a.stdv = P(mean), P(stdv)
            Y = sent(int(prow.max()) + 1, ldy)
            before, sbefore = Y.clone(), src.clone()
            a.Y, a.ldy, a.ymap = P(Y), ldy, (ci * 3)(*(MAP if mapped else (0, 0, 0)))
            call(lib, "m3pc_debug_head_out", a, kid, what)
            same(src, sbefore, what)
            out = owned(Y, before, prow, D, what)
            ref, B = R.head_out_ref(x, W, b, mean if detok else None, stdv if detok else None, mfma=mfma)
            hold(kid, "Y", out, ref, B, regime, what)


# ------------------------------------------------------------------------------------------------ critic
CRITIC_ROWS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 300)
CRITIC_SA = ((1, 1), (17, 6), (26, 6), (31, 1))


def _critic_cases():
    cs = [dict(name=f"critic_h{H}_S{S}_A{A}", H=H, S=S, A=A, rows=CRITIC_ROWS[i % 2::2] if (S, A) != (17, 6) else CRITIC_ROWS, both=True)
          for H in (64, 128, 256) for i, (S, A) in enumerate(CRITIC_SA)]
    cs += [dict(name=f"critic_scalar_h{H}_S{S}_A{A}", H=H, S=S, A=A, rows=(1, 17, 300), both=False)
           for H, S, A in ((32, 17, 6), (96, 26, 6), (64, 32, 32), (256, 32, 32))]
    return cs


CRITIC_CASES = _critic_cases()


@pytest.mark.parametrize("c", CRITIC_CASES, ids=[c["name"] for c in CRITIC_CASES])
def test_critic_against_float64(lib, c):
    H, S, A = c["H"], c["S"], c["A"]
    mf_id = {64: 20, 128: 21, 256: 22}.get(H)
    for ri, rows in enumerate(c["rows"]):
        for gi, regime in enumerate(REGIMES):
            what = f"{c['name']}_r{rows}/{regime}"
            states, actions, om, os_, nets = R.critic_inputs(regime, rows, S, A, H, DEV, 31 * rows + H + S + gi)
            st, ac = nan_rows(states, S), nan_rows(actions, A)  # (a NaN row behind the last)
            host = [[t.cpu().contiguous() for t in net] for net in nets]
            a = CriticArgs()
            a.states, a.actions, a.rows, a.S, a.A, a.hidden, a.om, a.os = P(st), P(ac), rows, S, A, H, P(om), P(os_)
            for j, name in enumerate(("W1", "b1", "W2", "b2", "W3", "b3")):
                src = host if name in ("W1", "W2") else nets
                setattr(a, name, (vp * 2)(P(src[0][j]), P(src[1][j])))
            outs = {}
            for force in (1, 0):  # (unforced, the dispatch itself keeps what the matrix-core kernel does not cover on the scalar one)
                kid = 19 if force or not c["both"] else mf_id
                q = sent(1, rows + 3)[0]
                before = q.clone()
                a.q, a.force_scalar = P(q), force
                call(lib, "m3pc_debug_critic", a, kid, what)
                after = q.clone()
                after[:rows] = before[:rows]
                assert torch.equal(_bits(after), _bits(before)), f"{what}: q was written behind row {rows - 1}"
                ref, B = R.critic_ref(states, actions, om, os_, nets, R.critic_n3(kid != 19, H))
                hold(kid, "q", q[:rows], ref, B, regime, what + f" kernel {kid}")
                outs[kid] = q[:rows].clone()
            if regime == "int" and c["both"]:
                assert torch.equal(_bits(outs[19]), _bits(outs[mf_id])), f"{what}: the scalar and the matrix-core kernel differ"


# ------------------------------------------------------------------------------------------------ actor head
ACTOR_CASES = [dict(name=f"actor_d{d}_A{A}", d=d, A=A) for d in (64, 256, 512, 1024) for A in (1, 4, 5, 8, 9, 32)]


@pytest.mark.parametrize("c", ACTOR_CASES, ids=[c["name"] for c in ACTOR_CASES])
def test_actor_head_against_float64(lib, c):
    d, A = c["d"], c["A"]
    fuses = d % 256 == 0 and A <= 8
    kid = (15 if A <= 4 else 16) if fuses else 17
    for ri, rows in enumerate((1, 4, 5, 129)):
        for ln in ((False, True) if fuses else (False,)):
            mapped = bool((ri + int(ln)) % 2)
            prow = R.map_rows(MAP if mapped else None, rows, DEV)
            ldx = d + (4 if ri % 2 else 0)
            for gi, regime in enumerate(REGIMES):
                what = f"{c['name']}_r{rows}" + ("_ln" if ln else "") + ("_map" if mapped else "") + f"/{regime}"
                x, Wmu, bmu, Wls, bls, lnp = R.actor_inputs(regime, rows, d, A, DEV, 13 * rows + d + A + gi, ln)
                X = nan_rows(x, ldx, prow)
                a = ActorArgs()
                a.X, a.ldx, a.rows, a.d, a.A = P(X), ldx, rows, d, A
                a.xmap = (ci * 3)(*(MAP if mapped else (0, 0, 0)))
                Wm, Wl = nan_rows(Wmu, d), nan_rows(Wls, d)  # (a NaN weight row behind row A - 1)
                a.Wmu, a.bmu, a.Wls, a.bls = P(Wm), P(bmu), P(Wl), P(bls)
                if ln:
                    a.ln_g, a.ln_b = P(lnp[0]), P(lnp[1])
                mu, sd = sent(rows, A), sent(rows, A)
                bm, bs, Xbefore = mu.clone(), sd.clone(), X.clone()
                a.mu, a.sd = P(mu), P(sd)
                call(lib, "m3pc_debug_actor_head", a, kid, what)
                same(X, Xbefore, what)
                r = torch.arange(rows, device=DEV)
                mu_o, sd_o = owned(mu, bm, r, A, what + " mu"), owned(sd, bs, r, A, what + " sd")
                rmu, Emu, rsd, Esd = R.actor_ref(x, Wmu, bmu, Wls, bls, lnp, norm=R.ln_int_ref if regime == "int" else R.layernorm64)
                hold(kid, "mu", mu_o, rmu, Emu, regime, what)
                hold(kid, "sd", sd_o, rsd, Esd, "randn" if regime == "int" else regime, what)  # (tanhf / expf: never exact)


# ------------------------------------------------------------------------------------------------ embed
EMBED_CASES = [dict(name=f"embed_d{d}_feat{f}" + ("_ln" if ln else ""), d=d, feat=f, ln=ln)
               for d in (64, 192, 320, 960, 256, 512, 768, 1024) for f in (1, 32) for ln in (False, True)]


@pytest.mark.parametrize("c", EMBED_CASES, ids=[c["name"] for c in EMBED_CASES])
def test_embed_against_float64(lib, c):
    """embed_kernel (d % 256 != 0: three waves at d = 192, 256 threads with two columns for some at d = 320, 960 = 3.75 columns a thread)
    and, with the same reference, embed_rows_kernel<1..4>: the row, and the fused LayerNorm of the kernel's own row in fp32 (Hf, through
    m3pc_debug_embed_ex) and bf16 (Hb).  int: integers, and with the norm the table rows E are ln_int_rows and every row of WT is constant,
    so that the token's features shift a row by an integer and its variance stays 256: row and norm are exact.  randn: rows of a standard
    deviation from 0.03 to 3 (a scale per step), the small ones for the eps.  offset: the same rows 300 of their standard deviations from
    zero, which is where a one-pass variance or a dropped centring shows."""
    d, feat, ln = c["d"], c["feat"], c["ln"]
    kid = 1 if d % 256 else 1 + d // 256
    batch, T = 3, 5
    tokmap = [(0, t) for t in range(T)] + [(1, t) for t in (0, T - 1)]  # key 0: `feat` features; key 1: 3 features
    L = len(tokmap)
    feats = (feat, 3)
    r = torch.arange(batch * L, device=DEV)
    for gi, regime in enumerate(REGIMES):
        what = f"{c['name']}/{regime}"
        rn, ri, _ = R.gen(DEV, 17 * d + feat + gi)
        if regime == "int":
            tok = [ri(-3, 3, batch, T, f) for f in feats]
            WT = [ri(-3, 3, f, 1).expand(f, d).contiguous() if ln else ri(-3, 3, f, d) for f in feats]
            E = [R.ln_int_rows(T, d, DEV, 3 * d + k) if ln else ri(-3, 3, T, d) for k in range(2)]
            g, b = ri(-4, 4, d), ri(-4, 4, d)
        else:
            sc = 10.0 ** torch.linspace(-1.5, 0.5, T, device=DEV)  # a scale per step, 0.03 .. 3: the eps of the norm shows in the small rows
            tok, WT = [rn(batch, T, f) * sc[None, :, None] for f in feats], [rn(f, d) for f in feats]
            E = [(rn(T, d) + (300.0 * (f + 1) ** 0.5 * torch.sign(rn(T, 1)) if regime == "offset" else 0.0)) * sc[:, None] for f in feats]
            g, b = 1 + 0.3 * rn(d), rn(d)
        tm = torch.tensor(tokmap, dtype=torch.int32, device=DEV)
        rows_ref, rows_B = [], []
        for bi in range(batch):
            for k, t in tokmap:
                v, B = R.embed_ref(tok[k][bi, t][None], WT[k], E[k][t][None])
                rows_ref.append(v[0])
                rows_B.append(B[0])
        ref, B = torch.stack(rows_ref), torch.stack(rows_B)
        Hb_both = None
        for outs in (("fb", "b") if ln else ("",)):
            ex = EmbedExArgs()
            a = ex.base
            a.tok, a.WT, a.E = (vp * 4)(P(tok[0]), P(tok[1]), None, None), (vp * 4)(P(WT[0]), P(WT[1]), None, None), (vp * 4)(P(E[0]), P(E[1]), None, None)
            a.bstride, a.feat = (ll * 4)(T * feats[0], T * feats[1], 0, 0), (ci * 4)(feats[0], feats[1], 0, 0)
            a.tokmap, a.batch, a.L, a.d, a.T = P(tm), batch, L, d, T
            X, Hf, Hb = sent(batch * L, d), sent(batch * L, d), sent(batch * L, d, torch.bfloat16)
            bx, bf, bh = X.clone(), Hf.clone(), Hb.clone()
            a.X = P(X)
            if ln:
                a.ln_g, a.ln_b, a.Hb = P(g), P(b), P(Hb)
                if "f" in outs:
                    ex.Hf = P(Hf)
            a.stream = stream()
            picked = (ci * 1)(-1)
            ex.picked = C.cast(picked, pi)
            assert lib.m3pc_debug_embed_ex(C.byref(ex)) == 0, (what, lib.m3pc_last_error())
            torch.cuda.synchronize()
            assert picked[0] == kid == lib.m3pc_debug_elementwise_picked(), f"{what}: the launcher reports kernel {picked[0]}, the case is for {kid}"
            REACHED.add(kid)
            Xo = owned(X, bx, r, d, what + " X")
            hold(kid, "X", Xo, ref, B, regime, what)
            if not ln:
                same(Hb, bh, what + " Hb without ln_g")
                same(Hf, bf, what + " Hf without ln_g")
                continue
            # the norm of the kernel's own fp32 row
            y, By = (R.ln_int_ref if regime == "int" else R.layernorm64)(Xo, g, b), R.ln_bound(Xo, g, b)
            Ho = owned(Hb, bh, r, d, what + " Hb")
            hold(kid, "Hb", Ho.float(), y, R.bf16_out_bound(y, By), regime, what)
            if "f" in outs:
                Fo = owned(Hf, bf, r, d, what + " Hf")
                hold(kid, "Hf", Fo, y, By, regime, what)
                assert torch.equal(_bits(Fo.to(torch.bfloat16)), _bits(Ho)), f"{what}: Hb is not the bf16 rounding of Hf"
                Hb_both = Ho.clone()
            else:
                same(Hf, bf, what + " Hf not asked for")
                assert torch.equal(_bits(Ho), _bits(Hb_both)), f"{what}: Hb alone differs from Hb beside Hf"


# ------------------------------------------------------------------------------------------------ sample
def _sample_cases():
    cs = []
    T, A = 6, 3
    for mode in (0, 1, 2):
        for ii, idx in enumerate((0, 1, T - 1)):
            k = mode * 3 + ii
            cs.append(dict(name=f"sample_mode{mode}_idx{idx}", mode=mode, T=T, A=A, idx=idx, n=37, widx=bool(k % 2), index=bool((k // 2) % 2),
                           sa=bool(k % 3 != 1), loc_out=bool(k % 2 == 0)))
    cs += [dict(name=f"sample_mode{mode}_past_the_grid_cap", mode=mode, T=8, A=4, idx=2, n=16385, widx=mode == 1, index=mode != 1, sa=True, loc_out=True)
           for mode in (0, 1, 2)]  # 16385 * 8 * 4 = 524320 > 2048 * 256
    return cs


SAMPLE_CASES = _sample_cases()


@pytest.mark.parametrize("c", SAMPLE_CASES, ids=[c["name"] for c in SAMPLE_CASES])
def test_sample_bit_for_bit(lib, c):
    """sample_kernel against sample_ref.  Everything around the tanh -- the history copy, the row and window indices, e * sd + loc with a
    rounding each, 0.09 e, the clamp, sample_actions -- is an independent float32 numpy restatement; the tanh itself is torch.tanh on the
    device, because the device library's tanhf has no bit-exact CPU twin.  The bit-for-bit claim of modes 0 and 1 therefore rests on torch's
    bundled device library being the tanhf build hipcc links: a ROCm / torch version skew would fail these cases for a reason outside the
    project (mode 2 and every t < idx involve no tanh)."""
    mode, T, A, idx, n = c["mode"], c["T"], c["A"], c["idx"], c["n"]
    h = T - idx
    rn, ri, g = R.gen(DEV, 5 + mode + idx + n)
    nwin, n_total, n_begin = (4 if c["widx"] else 1), n + 11, 5
    hist = torch.tanh(rn(nwin, T, A))
    loc, sd = rn(T, A), 0.1 + torch.rand(T, A, device=DEV, generator=g)
    eps = rn(n_total, T if mode == 0 else h, A)
    if mode == 2:
        eps = torch.tanh(eps)
    widx = torch.randint(0, nwin, (n,), device=DEV, generator=g, dtype=torch.int32) if c["widx"] else None
    index = torch.randint(0, n_total, (n,), device=DEV, generator=g, dtype=torch.int32) if c["index"] else None
    a = SampleArgs()
    a.hist_actions, a.loc, a.sd, a.eps = P(hist), P(loc), P(sd), P(eps)
    a.mode, a.T, a.A, a.idx, a.h, a.n_begin, a.n_count = mode, T, A, idx, h, n_begin, n
    a.widx, a.index, a.eps_rows, a.hist_windows = P(widx), P(index), n_total, nwin
    cand, sa = sent(n, T * A), sent(n, h * A)
    lo, so = sent(1, T * A), sent(1, T * A)
    before = [t.clone() for t in (cand, sa, lo, so)]
    a.cand = P(cand)
    if c["sa"]:
        a.sample_actions = P(sa)
    if c["loc_out"]:
        a.loc_out, a.sd_out = P(lo), P(so)
    call(lib, "m3pc_debug_sample", a, 18, c["name"])
    r = torch.arange(n, device=DEV)
    cand_o = owned(cand, before[0], r, T * A, c["name"] + " cand")
    dev_tanh = lambda x: torch.tanh(torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)).cpu().numpy()
    f = lambda t: None if t is None else t.cpu().numpy()
    rc, rs = R.sample_ref(f(hist), f(loc), f(sd), f(eps), mode, T, A, idx, h, n_begin, n, f(widx), f(index), tanh=dev_tanh)
    exact(18, cand_o, rc.reshape(n, T * A), c["name"] + " cand")
    if c["sa"]:
        exact(18, owned(sa, before[1], r, h * A, c["name"] + " sample_actions"), rs.reshape(n, h * A), c["name"] + " sample_actions")
    else:
        same(sa, before[1], c["name"] + " sample_actions")
    if c["loc_out"]:
        z = torch.zeros(1, dtype=torch.long, device=DEV)
        exact(18, owned(lo, before[2], z, T * A, c["name"] + " loc_out"), f(loc).reshape(1, -1), c["name"] + " loc_out")
        exact(18, owned(so, before[3], z, T * A, c["name"] + " sd_out"), f(sd).reshape(1, -1), c["name"] + " sd_out")
    else:
        same(lo, before[2], c["name"] + " loc_out")


# ------------------------------------------------------------------------------------------------ score
@pytest.mark.parametrize("h", (1, 2, 7, 64), ids=lambda h: f"score_h{h}")
def test_score_bit_for_bit_with_the_quadratic_loop(lib, h):
    """score_kernel's O(h) running form against the O(h^2) loop of the oracle's td_lambda, restated in float32."""
    k = 0
    for n in (1, 255, 256, 257):
        for boot_scale in (1.0, 1000.0):
            for lmbda in (0.0, 0.95, 1.0):
                k += 1
                scatter, boot_out = bool(k % 2), bool((k // 2) % 2)
                what = f"score_h{h}_n{n}_scale{boot_scale:g}_lmbda{lmbda:g}"
                rn, ri, g = R.gen(DEV, 1000 * h + n + k)
                rewards, boot = rn(n, h), rn(n, h) * (1.0 if boot_scale == 1.0 else 1e-3)
                a = ScoreArgs()
                a.rewards, a.boot, a.n, a.h, a.boot_scale, a.gamma, a.lmbda = P(rewards), P(boot), n, h, boot_scale, 0.99, lmbda
                er, bo, sc = sent(1, n + 3)[0], sent(n, h), sent(1, 2 * n + 3)[0]
                before = [t.clone() for t in (er, bo, sc)]
                sidx = (2 * torch.randperm(n, device=DEV, generator=g)).to(torch.int32)
                a.expect_return = P(er)
                if boot_out:
                    a.boot_out = P(bo)
                if scatter:
                    a.scatter_index, a.scatter_out = P(sidx), P(sc)
                call(lib, "m3pc_debug_score", a, 23, what)
                ref, rb = R.td_lambda_ref(rewards.cpu().numpy(), boot.cpu().numpy(), boot_scale, 0.99, lmbda)
                assert torch.equal(_bits(er[n:]), _bits(before[0][n:])), f"{what}: expect_return written behind row {n - 1}"
                exact(23, er[:n], ref, what)
                if boot_out:
                    exact(23, owned(bo, before[1], torch.arange(n, device=DEV), h, what + " boot_out"), rb, what + " boot_out")
                else:
                    same(bo, before[1], what + " boot_out")
                if scatter:
                    want = before[2].clone()
                    want[sidx.long()] = er[:n]
                    assert torch.equal(_bits(sc), _bits(want)), f"{what}: scatter_out"
                else:
                    same(sc, before[2], what + " scatter_out")


# ------------------------------------------------------------------------------------------------ gather_rows
@pytest.mark.parametrize("d", (64, 512, 1024), ids=lambda d: f"gather_d{d}")
def test_gather_rows_bit_for_bit(lib, d):
    batch, xe_rows, table_rows = 3, 5, 4
    rowsrc = [2, -1, 0, -4, 4, 4, -2]  # table rows and own rows mixed; the last own row and the last table row among them
    rn, _, _ = R.gen(DEV, d)
    Xe = torch.full((batch, xe_rows + 1, d), float("nan"), device=DEV)  # (a NaN row behind every batch element's rows)
    Xe[:, :xe_rows] = rn(batch, xe_rows, d)
    table = nan_rows(rn(table_rows, d), d)
    src = (ci * len(rowsrc))(*rowsrc)
    n = batch * len(rowsrc)
    want = R.gather_ref(Xe.cpu().numpy(), table.cpu().numpy(), rowsrc).reshape(n, d)
    for outs in ("f", "b", "fb"):
        what = f"gather_d{d}_{outs}"
        a = GatherArgs()
        a.Xe, a.xe_bstride, a.table, a.rowsrc = P(Xe), (xe_rows + 1) * d, P(table), C.cast(src, vp)
        a.rows_per_batch, a.batch, a.d, a.xe_rows, a.table_rows = len(rowsrc), batch, d, xe_rows, table_rows
        out, outb = sent(n, d), sent(n, d, torch.bfloat16)
        bo, bb = out.clone(), outb.clone()
        if "f" in outs:
            a.out = P(out)
        if "b" in outs:
            a.outb = P(outb)
        call(lib, "m3pc_debug_gather_rows", a, 6, what)
        r = torch.arange(n, device=DEV)
        if "f" in outs:
            exact(6, owned(out, bo, r, d, what + " out"), want, what)
        else:
            same(out, bo, what + " out")
        if "b" in outs:
            got = owned(outb, bb, r, d, what + " outb")
            assert torch.equal(_bits(got), _bits(torch.from_numpy(want).to(DEV).to(torch.bfloat16))), f"{what}: outb is not the bf16 rounding of the rows"
            EXACT[6] = EXACT.get(6, 0) + 1
        else:
            same(outb, bb, what + " outb")


# ------------------------------------------------------------------------------------------------ tokeniser, de-tokeniser, overlays
def _tok_stats(D, seed):
    rn, _, g = R.gen(DEV, seed)
    return rn(D), 0.5 + torch.rand(D, device=DEV, generator=g)


OVERLAY_CASES = [dict(name=f"overlay_D{D}_idx{i}", D=D, T=7, idx=i, windows=5) for D in (1, 17) for i in (0, 4, 5, 6)]  # idx 0, T - 3, T - 2, T - 1
OVERLAY_CASES.append(dict(name="overlay_past_the_grid_cap", D=17, T=16, idx=7, windows=2000))  # 544000 > 2048 * 256


@pytest.mark.parametrize("c", OVERLAY_CASES, ids=[c["name"] for c in OVERLAY_CASES])
def test_goal_overlays_bit_for_bit(lib, c):
    """goal_overlay_kernel with and without the de-tokeniser, and goal_overlay_rows_kernel with exactly the overlay rows per window
    (nq = their number) and with two unused rows behind them (nq + 2: the row stride of pred is nq, the unused rows hold NaN)."""
    D, T, idx, W = c["D"], c["T"], c["idx"], c["windows"]
    rn, _, _ = R.gen(DEV, 3 * D + idx)
    mean, stdv = _tok_stats(D, 50 + D)
    f = lambda t: t.cpu().numpy()
    r = torch.arange(W * T, device=DEV)
    picked = (ci * 1)(-1)
    sin = rn(W * T, D)
    sbefore = sin.clone()
    for nm in (True, False):  # the in-place form
        what = c["name"] + ("_norm" if nm else "")
        pred = rn(W * T, D)
        want_p, want_o = R.overlay_ref(f(pred).reshape(W, T, D), f(sin).reshape(W, T, D), T, idx, f(mean), f(stdv), nm)
        pbuf = torch.cat([pred, torch.full((1, D), SENT, device=DEV)])
        out = sent(W * T, D)
        before = out.clone()
        rc = lib.m3pc_debug_goal_overlay(P(pbuf), P(sin), P(out), W, T, D, idx, P(mean) if nm else None, P(stdv) if nm else None, int(nm), stream(), picked)
        assert rc == 0 and picked[0] == 26, (what, rc, picked[0], lib.m3pc_last_error())
        torch.cuda.synchronize()
        REACHED.add(26)
        same(sin, sbefore, what)
        assert float(pbuf[-1, 0]) == SENT, f"{what}: pred written behind its last row"
        exact(26, pbuf[:W * T], want_p.reshape(W * T, D), what + " pred")
        exact(26, owned(out, before, r, D, what + " states_out"), want_o.reshape(W * T, D), what + " states_out")
    n_over = int(R.overlay_rows_mask(T, idx).sum())
    for nq in (n_over, n_over + 2):  # the rows form: the overlay rows of every window, already de-tokenised
        what = f"{c['name']} rows form nq {nq}"
        predq = torch.full((W + 1, nq, D), float("nan"), device=DEV)  # (NaN in the unused rows and in a window behind the last)
        predq[:W, :n_over] = rn(W, n_over, D)
        want = R.overlay_rows_ref(f(predq)[:W], f(sin).reshape(W, T, D), T, idx)
        out = sent(W * T, D)
        before, pbefore = out.clone(), predq.clone()
        rc = lib.m3pc_debug_goal_overlay_rows(P(predq), P(sin), P(out), W, T, D, idx, nq, stream(), picked)
        assert rc == 0 and picked[0] == 27, (what, rc, picked[0], lib.m3pc_last_error())
        torch.cuda.synchronize()
        REACHED.add(27)
        same(predq, pbefore, what)
        exact(27, owned(out, before, r, D, what), want.reshape(W * T, D), what)


@pytest.mark.parametrize("normalize", (False, True), ids=("plain", "normalize"))
def test_tokeniser_bit_for_bit(lib, normalize):
    """tokenize_kernel / detokenize_kernel through m3pc_tokenize / m3pc_detokenize of a handle with 17 state features (key 0) and the
    one-feature rewards (key 2); f32 and f64 input; one launch each past the grid cap of 2048 * 256 elements."""
    from m3pc_amd import capi
    dims = capi.Dims(17, 3, 16, 64, 1, 1, 1, 64, 1, 256, 64, 0)
    h = vp()
    assert lib.m3pc_create(C.byref(dims), 0, C.byref(h)) == 0, lib.m3pc_last_error()
    try:
        fp = C.POINTER(C.c_float)
        for key, D in ((0, 17), (2, 1)):
            mean, stdv = _tok_stats(D, 70 + D)
            mh, sh = mean.cpu().contiguous(), stdv.cpu().contiguous()
            assert lib.m3pc_set_tokenizer(h, key, C.cast(mh.data_ptr(), fp), C.cast(sh.data_ptr(), fp), D, int(normalize)) == 0, lib.m3pc_last_error()
            for rows in (1, 5, 257, 524288 // D + 300):
                for et in (torch.float32, torch.float64):
                    what = f"tokenise_D{D}_rows{rows}_{'f64' if et == torch.float64 else 'f32'}"
                    x = (torch.randn(rows, D, device=DEV, dtype=torch.float64, generator=torch.Generator(device=DEV).manual_seed(rows + D)) * 3).to(et)
                    out = sent(rows, D)
                    before = out.clone()
                    assert lib.m3pc_tokenize(h, key, P(x), int(et == torch.float64), P(out), rows, stream()) == 0, lib.m3pc_last_error()
                    torch.cuda.synchronize()
                    assert lib.m3pc_debug_elementwise_picked() == 24
                    REACHED.add(24)
                    r = torch.arange(rows, device=DEV)
                    tk = owned(out, before, r, D, what)
                    exact(24, tk, R.tokenize_ref(x.cpu().numpy(), mh.numpy(), sh.numpy(), normalize), what)
                    if et == torch.float64:
                        continue
                    back = sent(rows, D)
                    before = back.clone()
                    tkc = tk.contiguous()
                    assert lib.m3pc_detokenize(h, key, P(tkc), P(back), rows, stream()) == 0, lib.m3pc_last_error()
                    torch.cuda.synchronize()
                    assert lib.m3pc_debug_elementwise_picked() == 25
                    REACHED.add(25)
                    exact(25, owned(back, before, r, D, what + " back"), R.detokenize_ref(tkc.cpu().numpy(), mh.numpy(), sh.numpy(), normalize), what + " back")
    finally:
        lib.m3pc_destroy(h)


# ------------------------------------------------------------------------------------------------ the table
def case_ids():
    """The kernel ids the case tables name (each launch asserts that the launcher reports its case's id)."""
    ids = {c["kid"] for c in LN_CASES} | {c["kid"] for c in HEAD_CASES} | {19}
    ids |= {{64: 20, 128: 21, 256: 22}[c["H"]] for c in CRITIC_CASES if c["both"]}
    ids |= {(15 if c["A"] <= 4 else 16) if c["d"] % 256 == 0 and c["A"] <= 8 else 17 for c in ACTOR_CASES}
    ids |= {1 if c["d"] % 256 else 1 + c["d"] // 256 for c in EMBED_CASES}
    # sample, score, gather_rows, the tokeniser pair and the two overlays: one kernel each
    return ids | {18, 23, 6, 24, 25, 26, 27}


def test_every_elementwise_kernel_has_a_case():
    """The cases name exactly the kernel ids of include/m3pc_hip_debug.h, and (when the module ran as a whole) every one of them was
    reported by a launch.  Prints the largest err / bound per kernel id seen in the randn and offset regimes and the number of exact
    comparisons (int regime, bit-for-bit kernels)."""
    want = header_ids()
    assert set(want) == set(range(1, 28)), sorted(want)
    have = case_ids()
    assert have == set(want), (sorted(set(want) - have), sorted(have - set(want)))
    if not WORST:
        return
    assert REACHED == set(want), f"kernel ids no launch reported: {sorted(set(want) - REACHED)}"
    print("\nlargest err / bound per kernel id (randn and offset regimes) | exact comparisons (int regime, bit for bit):")
    for kid in sorted(want):
        w = "  ".join(f"{k} {v:.3g}" for (i, k), v in sorted(WORST.items()) if i == kid)
        print(f"  {kid:2d} {want[kid]:30s} {w or '-':40s} | {EXACT.get(kid, 0)}")
