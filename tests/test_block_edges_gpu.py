"""Every form of the fused layer tail (m3pc_amd/csrc/block_fused.hip: block_fused_kernel<0, 0|1|2|3> and its bf16-residual
instances, block_split_reduce_kernel, kv_fused_kernel, the pack kernels) at its row and tile edges, stage by stage against the
float64 restatement of tests/block_ref.py, through the lab hooks m3pc_debug_block_ex / m3pc_debug_kv_fused_ex.

Each case names its form (the `picked` value the hook must report; the list is in include/m3pc_hip_debug.h), its row count, its
residual source and its outputs; test_every_block_form_has_a_case checks that the cases reach exactly the forms of that list, and
tests/test_block_ref_cpu.py holds the table to block_fused_accepts without a GPU.  Every case runs in the three regimes of block_ref:
`first` and `second` are exact, `random` checks X'' at the project's tolerance and everything behind it from the kernel's own X''.
Everything a kernel may not read holds NaN (padding columns of O and the residual rows, the shared leading rows of sequences >= 1,
table rows that have a row of their own behind the table); every output buffer holds a sentinel in its padding columns and in a
guard row behind it and is compared bit for bit with its state before the call outside the elements the call owns."""
import ctypes as C
import os
import re

import pytest
import torch

import block_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -31744.0  # exact in bf16 and fp32; no case comes near it
DEV = "cuda"
D, FF = R.D, R.FF
vp, ci = C.c_void_p, C.c_int


class BArgs(C.Structure):
    """m3pc_debug_block_args (include/m3pc_hip_debug.h)."""
    _fields_ = [("O", vp), ("ldo", ci), ("M", ci), ("res", vp), ("ldr", ci), ("res_L", ci), ("res_nshared", ci), ("rowtab", vp),
                ("rt_mod", ci), ("res_nu", ci), ("Wo", vp), ("W1", vp), ("W2", vp), ("Wqkv", vp), ("Wh", vp), ("stream_buf", vp),
                ("bo", vp), ("b1", vp), ("b2", vp), ("ln2_g", vp), ("ln2_b", vp), ("lnA_g", vp), ("lnA_b", vp), ("lnB_g", vp * 2),
                ("lnB_b", vp * 2), ("Xout", vp), ("ldx", ci), ("x_bf16", ci), ("Hout", vp), ("ldh", ci), ("out_mod", ci), ("out_grp", ci),
                ("QKVout", vp), ("ldq", ci), ("qkv_bytes", C.c_longlong), ("bqkv", vp), ("hb1", vp), ("hw2", vp), ("hb2", vp),
                ("hmean", vp), ("hstd", vp), ("head_out", vp * 2), ("split", ci), ("red_Xout", vp), ("red_ldx", ci), ("red_Hout", vp),
                ("red_ldh", ci), ("red_lnA_g", vp), ("red_lnA_b", vp), ("red_lnB_g", vp * 2), ("red_lnB_b", vp * 2), ("red_out_mod", ci),
                ("red_out_grp", ci), ("stream", vp), ("picked", C.POINTER(ci))]


class KArgs(C.Structure):
    """m3pc_debug_kv_args."""
    _fields_ = [("Z", vp), ("ldz", ci), ("M", ci * 2), ("map", (ci * 3) * 2), ("rowtab", vp * 2), ("rt_mod", ci * 2), ("We", vp * 2),
                ("Wkv", vp), ("stream_buf", vp), ("ln_g", vp), ("ln_b", vp), ("bkv", vp), ("KV", vp), ("ldkv", ci),
                ("kv_bytes", C.c_longlong), ("stream", vp)]


def case(name, form, M, out, src="res", res_L=0, res_nshared=0, rt_mod=0, res_nu=0, lnB=False, out_mod=0, out_grp=0, pad=False,
         detok=False, red=None, inplace=False):
    """out: letters X (X'' stored), H (Hout), Q (the next layer's Q|K|V), D (the two scalar heads).  src: "res" (with res_L /
    res_nshared: shared leading rows) or "tab" (rt_mod, res_nu).  red (split forms): what the reduce writes -- "X", "A" (Hout, lnA only)
    or "AB" (Hout, lnA, lnB, and row groups where out_mod is set).  inplace: also run with Xout aliasing the residual rows."""
    return dict(name=name, form=form, M=M, out=out, src=src, res_L=res_L, res_nshared=res_nshared, rt_mod=rt_mod, res_nu=res_nu, lnB=lnB,
                out_mod=out_mod, out_grp=out_grp, pad=pad, detok=detok, red=red, inplace=inplace, xb=form >= 16)


def _cases():
    cs = []
    # ---- plain, next-Q|K|V and their bf16-residual instances: fewer rows than a tile, a full tile, one row past it, three tiles
    for form, tag, out in ((0, "plain", "XH"), (1, "qkv", "XQ"), (16, "plain_xb", "XH"), (17, "qkv_xb", "XQ")):
        for M in (1, 31, 127, 128, 129, 300):
            cs.append(case(f"{tag}_m{M}", form, M, out, pad=M in (31, 129), inplace=True))
    # (the same forms when nothing needs X'': the last encoder layer, a consumed residual stream)
    cs += [case("plain_noX_m129", 0, 129, "H"), case("plain_xb_noX_m127", 16, 127, "H", pad=True), case("qkv_noX_m129", 1, 129, "Q", pad=True),
           case("qkv_xb_noX_m31", 17, 31, "Q")]
    # ---- shared leading residual rows of the candidate pass, output to another buffer
    for L, ns, n in ((49, 32, 3), (7, 3, 19), (7, 7, 19), (7, 0, 19)):
        for form, out in ((0, "XH"), (1, "XQ")):
            cs.append(case(f"shared_L{L}_ns{ns}_{out}", form, L * n, out, res_L=L, res_nshared=ns, pad=ns == 3))
    # ---- decoder forms: residual from a row table, rows with a residual of their own behind it
    for nq, n in ((32, 4), (10, 13), (1, 129)):
        for nu in sorted({0, 1, 2, nq} & set(range(nq + 1))):
            cs.append(case(f"tab_nq{nq}_nu{nu}_X", 0, nq * n, "X", src="tab", rt_mod=nq, res_nu=nu))
            if nq % 2 == 0:
                cs.append(case(f"tab_nq{nq}_nu{nu}_groups", 0, nq * n, "H", src="tab", rt_mod=nq, res_nu=nu, lnB=True, out_mod=nq, out_grp=nq // 2,
                               pad=nu == 1))
            cs.append(case(f"tab_nq{nq}_nu{nu}_onegroup", 0, nq * n, "H", src="tab", rt_mod=nq, res_nu=nu, lnB=True))
    # ---- the two scalar heads inside the tail: M / 2 = 1, 65, 128, 130 rows per head
    for n, hh in ((1, 1), (13, 5), (8, 16), (26, 5)):
        for detok in (False, True):
            for nu in (0, min(3, 2 * hh)):
                cs.append(case(f"heads_n{n}_h{hh}_nu{nu}" + ("_detok" if detok else ""), 2, 2 * hh * n, "D", src="tab", rt_mod=2 * hh, res_nu=nu,
                               lnB=True, out_mod=2 * hh, out_grp=hh, detok=detok))
    # ---- four workgroups per tile + the reduce
    for M in (1, 127, 129, 300):
        for src in ("res", "tab"):
            for red in ("X", "A", "AB"):
                groups = red == "AB" and M % 10 == 0
                cs.append(case(f"split_m{M}_{src}_{red}", 3, M, "X", src=src, rt_mod=(10 if M % 10 == 0 else 7) if src == "tab" else 0, red=red,
                               out_mod=10 if groups else 0, out_grp=5 if groups else 0, pad=red == "A"))
    return cs


CASES = _cases()
# kv_fused: (name, n, Le, kept, off, rt_mod, pad): group g holds the kept[g] rows at offset off[g] of each of n sequences of Le rows
KV_CASES = [("kv_1_3", 1, 5, (1, 3), (0, 2), (1, 3), False), ("kv_127_254", 127, 4, (1, 2), (0, 2), (1, 2), True),
            ("kv_128_alone", 64, 5, (2, 0), (1, 0), (2, 1), True), ("kv_129_129", 43, 7, (3, 3), (0, 4), (5, 2), False),
            ("kv_128_128", 32, 9, (4, 4), (0, 5), (2, 8), True)]
WORST = {}   # (form, stage) -> largest err / bound of the random regime
EXACT = [0]  # first / second runs
OFFSETS = []
# residual offset | path | X'' rows: mean |row mean| / row sd, largest fp32 error (beyond half a bf16 ulp of the output), err / bound | the same for
# the row whose X' is constant
OFFSET_FMT = "offset %2d sd  %-26s |mean| / sd %5.3g  fp32 err %.3g  err / bound %.3g   constant-X' row: |mean| / sd %5.3g  fp32 err %.3g  err / bound %.3g"


def header_forms():
    src = open(os.path.join(ROOT, "include", "m3pc_hip_debug.h")).read()
    block = src[src.index("Block forms"):src.index("the timing variants DBG")]
    return {int(x) for x in re.findall(r"(?:^|;|\*)\s*(\d+) block_fused_kernel", block, re.M)}


def lab():
    from hip_util import lab_library
    lib = lab_library()
    for fn in (lib.m3pc_debug_block_ex, lib.m3pc_debug_block_accepts):
        fn.restype, fn.argtypes = ci, [C.POINTER(BArgs)]
    lib.m3pc_debug_kv_fused_ex.restype, lib.m3pc_debug_kv_fused_ex.argtypes = ci, [C.POINTER(KArgs)]
    lib.m3pc_debug_block_stream_bytes.restype = C.c_longlong
    lib.m3pc_debug_kv_stream_bytes.restype = C.c_longlong
    return lib


def layout(c):
    """Leading dimensions and buffer row counts of a case."""
    p, xb, M = c["pad"], c["xb"], c["M"]
    ldr = (520 if xb else 516) if p else 512
    nseq = (M + c["rt_mod"] - 1) // c["rt_mod"] if c["rt_mod"] else 0
    return dict(ldo=520 if p else 512, ldr=ldr, ldx=512 if c["red"] else ldr, ldh=520 if p else 512, ldq=1544 if p else 1536,
                red_ldx=516 if p else 512, red_ldh=520 if p else 512, tab_rows=c["rt_mod"] + nseq * c["res_nu"], x_rows=(4 if c["red"] else 1) * M)


def fill_args(c, L, ptr, picked=None, inplace=False):
    """The hook's argument structure; ptr maps a buffer name to its address (the accepts-only entry never follows them)."""
    a = BArgs()
    a.O, a.ldo, a.M = ptr("O"), L["ldo"], c["M"]
    if c["src"] == "tab":
        a.rowtab, a.rt_mod, a.res_nu = ptr("tab"), c["rt_mod"], c["res_nu"]
    else:
        a.res, a.ldr, a.res_L, a.res_nshared = ptr("res"), L["ldr"], c["res_L"], c["res_nshared"]
    a.Wo, a.W1, a.W2, a.stream_buf = ptr("Wo"), ptr("W1"), ptr("W2"), ptr("stream")
    for k in ("bo", "b1", "b2"):
        setattr(a, k, ptr(k))
    a.ln2_g, a.ln2_b = ptr("g2"), ptr("be2")
    out = c["out"]
    if set(out) & set("HQD"):
        a.lnA_g, a.lnA_b = ptr("gA"), ptr("bA")
    if c["lnB"] and not c["red"]:
        a.lnB_g, a.lnB_b = (vp * 2)(ptr("lnB0"), ptr("lnB2")), (vp * 2)(ptr("lnB1"), ptr("lnB3"))
        a.out_mod, a.out_grp = c["out_mod"], c["out_grp"]
    a.x_bf16 = int(c["xb"])
    if "X" in out:
        a.Xout, a.ldx = ptr("res" if inplace else "X"), L["ldr"] if inplace else L["ldx"]
    if "H" in out:
        a.Hout, a.ldh = ptr("H"), L["ldh"]
    if "Q" in out:
        a.QKVout, a.ldq, a.qkv_bytes, a.bqkv, a.Wqkv = ptr("Q"), L["ldq"], c["M"] * L["ldq"] * 2, ptr("bqkv"), ptr("Wqkv")
    if "D" in out:
        a.Wh, a.hb1, a.hw2, a.hb2 = ptr("Wh"), ptr("hb1"), ptr("hw2"), ptr("hb2")
        if c["detok"]:
            a.hmean, a.hstd = ptr("hmean"), ptr("hstd")
        a.head_out = (vp * 2)(ptr("head0"), ptr("head1"))
    if c["red"]:
        a.split = 1
        if c["red"] == "X":
            a.red_Xout, a.red_ldx = ptr("redX"), L["red_ldx"]
        else:
            a.red_Hout, a.red_ldh, a.red_lnA_g, a.red_lnA_b = ptr("redH"), L["red_ldh"], ptr("gA"), ptr("bA")
        if c["red"] == "AB":
            a.red_lnB_g, a.red_lnB_b = (vp * 2)(ptr("lnB0"), ptr("lnB2")), (vp * 2)(ptr("lnB1"), ptr("lnB3"))
            a.red_out_mod, a.red_out_grp = c["out_mod"], c["out_grp"]
    if picked is not None:
        a.picked = C.cast(picked, C.POINTER(ci))
    return a


_NAMES = {}


def fake_ptr(name):
    """Distinct, 1 KiB-aligned addresses for the accepts-only entry."""
    return 0x10000000 + 0x1000000 * _NAMES.setdefault(name, len(_NAMES))


def accepts_of(lib, c, edit=None):
    picked = (ci * 1)()
    a = fill_args(c, layout(c), fake_ptr, picked)
    for k, v in (edit or {}).items():
        v = v(a) if callable(v) else v
        setattr(a, k, (vp * 2)(*v) if isinstance(v, tuple) else v)
    return lib.m3pc_debug_block_accepts(C.byref(a)), picked[0]


def refusal_cases():
    """(what, accepted case, one edit of its argument structure): everything block_fused_accepts refuses."""
    by = {c["name"]: c for c in CASES}
    plain, qkv, xb, tab = by["plain_m129"], by["qkv_m129"], by["plain_xb_m129"], by["tab_nq10_nu2_groups"]
    shared, heads, split, onegrp = by["shared_L7_ns3_XH"], by["heads_n13_h5_nu3"], by["split_m129_res_A"], by["tab_nq10_nu2_onegroup"]
    return [
        ("O off 16 bytes", plain, {"O": lambda a: a.O + 2}),
        ("ldo % 8", plain, {"ldo": 516}),
        ("ldr % 4", plain, {"ldr": 514}),
        ("ldx % 4", plain, {"ldx": 514}),
        ("ldh % 4", plain, {"ldh": 514}),
        ("ldq % 8", qkv, {"ldq": 1540}),
        ("ldq < 1536", qkv, {"ldq": 1528}),
        ("x_bf16 with ldr % 8", xb, {"ldr": 524}),
        ("x_bf16 with ldx % 8", xb, {"ldx": 524}),
        ("res_L with rowtab", tab, {"res_L": 5}),
        ("res_L in place", shared, {"Xout": lambda a: a.res}),
        ("res_nshared > res_L", shared, {"res_nshared": 8}),
        ("res_nu without rowtab", plain, {"res_nu": 1}),
        ("res_nu above rt_mod", tab, {"res_nu": 11}),
        ("res_nu with split", by["split_m129_tab_X"], {"res_nu": 1}),
        ("out_mod != 2 out_grp", tab, {"out_grp": 2}),
        ("M % out_mod", tab, {"M": 125}),
        ("heads with odd M", heads, {"M": 129}),
        ("heads without lnB", heads, {"lnB_g": (None, None), "lnB_b": (None, None)}),
        ("heads with Xout", heads, {"Xout": lambda a: fake_ptr("X"), "ldx": 512}),
        ("split with Hout", split, {"Hout": lambda a: fake_ptr("H"), "ldh": 512, "lnA_g": lambda a: fake_ptr("gA"), "lnA_b": lambda a: fake_ptr("bA")}),
        ("split in place", split, {"Xout": lambda a: a.res}),
        ("split with ldx != 512", split, {"ldx": 516}),
        ("qkv_bytes below M ldq 2", qkv, {"qkv_bytes": 129 * 1544 * 2 - 2}),
        ("x_bf16 with rowtab", onegrp, {"x_bf16": 1}),
    ]


# ------------------------------------------------------------------------------------------------ running a case
_PRM, _STREAM = {}, {}


def params(regime):
    """Weights and vectors of a regime on the device, with the bf16 copies the hook takes: built once, shared by every case."""
    if regime not in _PRM:
        prm = R.make_params(regime, DEV, seed=11 + R.REGIMES.index(regime))
        b = lambda t: t.to(torch.bfloat16).contiguous()
        dev = {"Wo": b(prm["W"]["o"]), "W1": b(prm["W"]["1"]), "W2": b(prm["W"]["2"]), "Wqkv": b(prm["W"]["qkv"]), "Wh": b(prm["W"]["h"]),
               "bqkv": prm["bqkv"], "We0": b(prm["We"][0]), "We1": b(prm["We"][1]), "Wkv": b(prm["Wkv"])}
        dev.update({k: prm["p"][k] for k in prm["p"]})
        dev.update({f"lnB{i}": prm["lnB"][i] for i in range(4)})
        dev.update({k: prm["heads"][k].contiguous() for k in prm["heads"]})
        _PRM[regime] = (prm, dev)
    return _PRM[regime]


def stream_buf(lib):
    if "b" not in _STREAM:
        _STREAM["b"] = torch.empty(int(lib.m3pc_debug_block_stream_bytes()), dtype=torch.uint8, device=DEV)
        _STREAM["kv"] = torch.empty(2 * int(lib.m3pc_debug_kv_stream_bytes()), dtype=torch.uint8, device=DEV)
    return _STREAM


def _nan(rows, ld, et=torch.float32):
    return torch.full((rows, ld), float("nan"), device=DEV, dtype=et)


def _sent(rows, ld, et=torch.float32):
    return torch.full((rows, ld), SENT, device=DEV, dtype=et)


def build(c, regime, seed, rows=None):
    """Logical rows (O, src: the physical residual rows / the table with the own rows behind it; rows: given instead of drawn) and the
    poisoned device buffers."""
    M, L = c["M"], layout(c)
    n_src = L["tab_rows"] if c["src"] == "tab" else M
    O, src = R.make_rows(regime, M, n_src, DEV, seed, x_bf16=c["xb"]) if rows is None else (rows[0].clone(), rows[1].clone())
    nan = float("nan")
    if regime == "first" and rows is None and c["src"] == "res" and not (c["res_L"] and (M - 1) % c["res_L"] < c["res_nshared"]):
        O[M - 1], src[M - 1] = 0.0, R.quiet_row(params(regime)[0])  # (the last row: a low-variance X'' row, block_ref.quiet_row)
    if c["src"] == "tab":
        src[:c["res_nu"]] = nan  # (table rows whose every user has a row of its own)
    elif c["res_L"]:
        r = torch.arange(M, device=DEV)
        src[(r >= c["res_L"]) & (r % c["res_L"] < c["res_nshared"])] = nan  # (stored once, in sequence 0)
    rt = torch.bfloat16 if c["xb"] else torch.float32
    bufs = {"O": _nan(M + 1, L["ldo"], torch.bfloat16)}
    bufs["O"][:M, :D] = O.to(torch.bfloat16)
    if c["src"] == "tab":
        bufs["tab"] = torch.cat([src, _nan(1, D)])
    else:
        bufs["res"] = _nan(M + 1, L["ldr"], rt)
        bufs["res"][:M, :D] = src.to(rt)
    out = c["out"]
    if "X" in out:
        bufs["X"] = _sent(L["x_rows"] + 1, L["ldx"], rt)
    if "H" in out:
        bufs["H"] = _sent(M + 1, L["ldh"], torch.bfloat16)
    if "Q" in out:
        bufs["Q"] = _sent(M + 1, L["ldq"], torch.bfloat16)
    if "D" in out:
        bufs["head0"], bufs["head1"] = _sent(1, M // 2 + 1)[0], _sent(1, M // 2 + 1)[0]
    if c["red"] == "X":
        bufs["redX"] = _sent(M + 1, L["red_ldx"])
    elif c["red"]:
        bufs["redH"] = _sent(M + 1, L["red_ldh"], torch.bfloat16)
    return O, src, L, bufs


def launch(lib, c, L, bufs, dev, inplace=False):
    picked = (ci * 1)(-1)
    sb = stream_buf(lib)["b"]
    ptr = lambda n: (sb if n == "stream" else bufs[n] if n in bufs else dev[n]).data_ptr()
    a = fill_args(c, L, ptr, picked, inplace=inplace)
    a.stream = torch.cuda.current_stream().cuda_stream
    rc = lib.m3pc_debug_block_ex(C.byref(a))
    assert rc == 0, (c["name"], lib.m3pc_last_error())
    torch.cuda.synchronize()
    assert picked[0] == c["form"], f"{c['name']}: the launcher reports form {picked[0]}, the case is for {c['form']}"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def untouched(buf, before, rows, ncols, what):
    """Outside [rows, :ncols] the buffer has the bits it had before the call."""
    after = buf.clone()
    if buf.dim() == 1:
        after[rows] = before[rows]
    else:
        after[rows, :ncols] = before[rows, :ncols]
    assert torch.equal(_bits(after), _bits(before)), f"{what}: a padding column, a guard row or a row of no owner was written"


def outputs(c, L, bufs, before, what):
    """Logical outputs of a finished launch; every guard checked."""
    M = c["M"]
    rows = torch.arange(M, device=DEV)
    o = {}
    if "X" in c["out"] and not c["red"]:
        untouched(bufs["X"], before["X"], rows, D, what + " Xout")
        o["X"] = bufs["X"][:M, :D].float()
    if "H" in c["out"]:
        untouched(bufs["H"], before["H"], rows, D, what + " Hout")
        _, hrow = R.group_of(M, c["out_mod"] if c["lnB"] else 0, c["out_grp"], DEV)
        o["H"] = bufs["H"][hrow, :D].float()
    if "Q" in c["out"]:
        untouched(bufs["Q"], before["Q"], rows, 3 * D, what + " QKV")
        o["QKV"] = bufs["Q"][:M, :3 * D].float()
    if "D" in c["out"]:
        for s in range(2):
            untouched(bufs[f"head{s}"], before[f"head{s}"], rows[:M // 2], 0, what + f" head {s}")
        o["heads"] = [bufs[f"head{s}"][:M // 2] for s in range(2)]
    for k, v in o.items():
        for t in (v if isinstance(v, list) else [v]):
            assert not bool((t == SENT).any()), f"{what}: an element of {k} was not written"
    return o


def companion(c):
    """The fp32-row launch of the same inputs that stores X'' (for forms that store none, or store it in bf16)."""
    out = "".join(sorted(set(c["out"].replace("D", "")) | {"X"}))
    return dict(c, out=out, form=1 if "Q" in out else 0, xb=False, lnB=c["lnB"] and "H" in out, red=None, name=c["name"] + "+X")


def run_case(lib, c, regime, seed):
    prm, dev = params(regime)
    what = f"{c['name']}/{regime}"
    O, src, L, bufs = build(c, regime, seed)
    before = {k: v.clone() for k, v in bufs.items()}
    launch(lib, c, L, bufs, dev)
    kw = dict(res_L=c["res_L"], res_nshared=c["res_nshared"], rt_mod=c["rt_mod"], res_nu=c["res_nu"])
    bk = dict(lnA=bool(set(c["out"]) & set("HQD")), lnB=c["lnB"], out_mod=c["out_mod"] if c["lnB"] else 0, out_grp=c["out_grp"], qkv="Q" in c["out"],
              heads="D" in c["out"], detok=c["detok"])
    ref = R.tail_ref(prm, O, src, x_bf16=c["xb"], **kw, **bk)
    for k in ("O", "res", "tab"):  # (inputs are inputs)
        if k in bufs:
            assert torch.equal(_bits(bufs[k]), _bits(before[k])), f"{what}: {k} was written"
    M = c["M"]
    if c["red"]:
        return run_split(lib, c, regime, prm, dev, ref, O, src, L, bufs, before, kw, what)
    o = outputs(c, L, bufs, before, what)
    if "X" in o and not c["xb"]:
        o["Xown"] = o["X"]
    else:
        cc = companion(c)
        Lc = layout(cc)
        _, _, _, cb = build(cc, regime, seed, rows=(O, src))
        cbefore = {k: v.clone() for k, v in cb.items()}
        launch(lib, cc, Lc, cb, dev)
        oc = outputs(cc, Lc, cb, cbefore, what + " (companion)")
        o["Xown"] = oc["X"]
        for k in ("H", "QKV"):  # the same X'' bits in both forms: whatever both store has the same bits
            if k in o and k in oc:
                assert torch.equal(o[k], oc[k]), f"{what}: {k} differs from the launch that also stores X''"
    res = R.check_tail(regime, prm, ref, o, what, x_bf16=c["xb"], **bk)
    if c["inplace"]:  # Xout aliasing the residual rows: the same bits, and the rows' padding and guard row stay NaN
        _, _, _, ib = build(c, regime, seed, rows=(O, src))
        ibefore = {k: v.clone() for k, v in ib.items()}
        launch(lib, c, L, ib, dev, inplace=True)
        untouched(ib["res"], ibefore["res"], torch.arange(M, device=DEV), D, what + " in place")
        assert torch.equal(_bits(ib["res"][:M, :D]), _bits(bufs["X"][:M, :D])), f"{what}: in place differs from out of place"
        for k in ("H", "Q"):
            if k in ib:
                assert torch.equal(_bits(ib[k]), _bits(bufs[k])), f"{what}: {k} in place differs from out of place"
    return res


def run_split(lib, c, regime, prm, dev, ref, O, src, L, bufs, before, kw, what):
    M = c["M"]
    untouched(bufs["X"], before["X"], torch.arange(4 * M, device=DEV), D, what + " slabs")
    slabs = bufs["X"][:4 * M].view(4, M, D)
    assert bool(torch.isfinite(slabs).all()) and not bool((slabs == SENT).any()), f"{what}: a slab element is missing"
    total = ((slabs[0] + slabs[1]) + slabs[2]) + slabs[3]  # (the reduce's order: fp32, slab by slab)
    o = {"Xown": total}
    groups = c["red"] == "AB"
    bk = dict(lnA=c["red"] != "X", lnB=groups, out_mod=c["out_mod"] if groups else 0, out_grp=c["out_grp"])
    rows = torch.arange(M, device=DEV)
    if c["red"] == "X":
        untouched(bufs["redX"], before["redX"], rows, D, what + " reduce Xout")
        o["X"] = bufs["redX"][:M, :D]
        assert torch.equal(_bits(o["X"]), _bits(total)), f"{what}: the reduce's Xout is not the sum of the slabs in slab order"
    else:
        untouched(bufs["redH"], before["redH"], rows, D, what + " reduce Hout")
        _, hrow = R.group_of(M, bk["out_mod"], bk["out_grp"], DEV)
        o["H"] = bufs["redH"][hrow, :D].float()
        assert not bool((o["H"] == SENT).any()), f"{what}: a row of the reduce's Hout was not written"
    res = R.check_tail(regime, prm, ref, o, what, one_pass=False, **bk)
    if regime == "random":  # the un-split launch of the same inputs, held to the same reference
        cc = dict(c, red=None, form=0, pad=False, out_mod=0, out_grp=0, name=c["name"] + " (un-split)")
        Lc = layout(cc)
        _, _, _, cb = build(cc, regime, 0, rows=(O, src))
        cbefore = {k: v.clone() for k, v in cb.items()}
        launch(lib, cc, Lc, cb, dev)
        oc = outputs(cc, Lc, cb, cbefore, what + " (un-split)")
        oc["Xown"] = oc["X"]
        R.check_tail(regime, prm, ref, oc, what + " (un-split)", lnA=False)
    return res


@pytest.fixture(scope="module")
def lib():
    return lab()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_block_form_against_float64(lib, i):
    c = CASES[i]
    rc, planned = accepts_of(lib, c)
    assert rc == 0 and planned == c["form"], (c["name"], rc, planned, lib.m3pc_last_error())
    for ri, regime in enumerate(R.REGIMES):
        res = run_case(lib, c, regime, 1000 * i + ri)
        if regime == "random":
            for k, v in res.items():
                WORST[(c["form"], k)] = max(WORST.get((c["form"], k), 0.0), v)
        else:
            EXACT[0] += 1
        print(f"{c['name']:32s} {regime:6s} form {c['form']:2d}  " + ("exact" if regime != "random" else
              "  ".join(f"{k} {v:.3g}" for k, v in res.items())))


# ------------------------------------------------------------------------------------------------ kv_fused
@pytest.mark.parametrize("name,n,Le,kept,off,rt_mod,pad", KV_CASES, ids=[k[0] for k in KV_CASES])
def test_kv_fused_against_float64(lib, name, n, Le, kept, off, rt_mod, pad):
    ldz, ldkv = (520, 1032) if pad else (512, 1024)
    rows = n * Le
    for ri, regime in enumerate(("second", "random")):
        prm, dev = params(regime)
        rn, _ = R._gen(DEV, 77 + ri + n)
        Zv = rn(rows, D).to(torch.bfloat16)
        Z = _nan(rows + 1, ldz, torch.bfloat16)
        Z[:rows, :D] = Zv
        tabs = [rn(max(rt_mod[g], 1), D) * 0.5 for g in range(2)]
        Ms = [n * kept[g] for g in range(2)]
        maps = [(kept[g], Le, off[g]) for g in range(2)]
        refs = [R.kv_ref(prm, Zv.float(), Ms[g], maps[g], rt_mod[g], g, tabs[g]) if Ms[g] else None for g in range(2)]
        last = max(int(r["prow"].max()) for r in refs if r is not None)
        KV = _sent(rows + 1, ldkv, torch.bfloat16)
        before = KV.clone()
        a = KArgs()
        a.Z, a.ldz, a.M = Z.data_ptr(), ldz, (ci * 2)(*Ms)
        for g in range(2):
            a.map[g] = (ci * 3)(*maps[g])
        a.rowtab, a.rt_mod = (vp * 2)(*[t.data_ptr() for t in tabs]), (ci * 2)(*rt_mod)
        a.We, a.Wkv, a.stream_buf = (vp * 2)(dev["We0"].data_ptr(), dev["We1"].data_ptr()), dev["Wkv"].data_ptr(), stream_buf(lib)["kv"].data_ptr()
        a.ln_g, a.ln_b, a.bkv = prm["ln_g"].data_ptr(), prm["ln_b"].data_ptr(), prm["bkv"].data_ptr()
        a.KV, a.ldkv, a.kv_bytes = KV.data_ptr(), ldkv, (last * ldkv + 2 * D) * 2  # (ends exactly behind the last mapped row)
        a.stream = torch.cuda.current_stream().cuda_stream
        assert lib.m3pc_debug_kv_fused_ex(C.byref(a)) == 0, lib.m3pc_last_error()
        torch.cuda.synchronize()
        owned = torch.cat([r["prow"] for r in refs if r is not None])
        assert owned.unique().numel() == owned.numel()
        untouched(KV, before, owned, 2 * D, f"{name}/{regime}")
        for g in range(2):
            if refs[g] is not None:
                w = R.check_kv(regime, refs[g], KV[refs[g]["prow"], :2 * D].float(), f"{name}/{regime} group {g}")
                WORST[("kv", "KV")] = max(WORST.get(("kv", "KV"), 0.0), w)
        print(f"{name:16s} {regime:6s} rows {Ms}  " + ("exact" if regime == "second" else f"max err / {R.KV_TOL[0]} {WORST[('kv', 'KV')]:.3g}"))


# ------------------------------------------------------------------------------------------------ row offsets
def test_layernorms_of_rows_with_a_large_mean(lib):
    """The fused tail's LayerNorms take the variance as E[x^2] - mean^2 from one pass, the split path's reduce takes it from the centred
    values.  Residual rows with a mean of 0, 8 and 32 row standard deviations (and one exactly constant row): Hout stays finite and
    within the one-pass (two-pass) bound of the float64 LayerNorm of the launch's own X''; the measured errors are printed."""
    regime, M = "random", 129
    prm, dev = params(regime)
    dev = dict(dev, bo=torch.zeros(D, device=DEV))  # (so that the constant row is constant in X' too)
    prm = dict(prm, p=dict(prm["p"], bo=dev["bo"]))
    for off in (0, 8, 32):
        O, src = R.make_rows(regime, M, M, DEV, 5)
        src = src + off * float(src.std())
        O[77], src[77] = 0.0, 3.0 + off
        for split in (False, True):
            c = case(f"offset{off}", 3 if split else 0, M, "X" if split else "XH", red="A" if split else None)
            L = layout(c)
            _, _, _, bufs = build(c, regime, 0, rows=(O, src))
            launch(lib, c, L, bufs, dev)
            if split:
                s = bufs["X"][:4 * M].view(4, M, D)
                X, H = ((s[0] + s[1]) + s[2]) + s[3], bufs["redH"][:M, :D].double()
            else:
                X, H = bufs["X"][:M, :D], bufs["H"][:M, :D].double()
            assert bool(torch.isfinite(X).all()) and bool(torch.isfinite(H).all())
            if not split:
                ref = R.tail_ref(prm, O, src)
                assert float((X.double() - ref["x2"]).abs().max()) <= R.X_RTOL * float(ref["x2"].abs().max())
            own = R.behind(X, prm, one_pass=not split)
            err, ratio = (H - own["y"]).abs(), ((H - own["y"]).abs() / own["Hb"])
            f32 = (err - R.half_ulp_bf16(own["y"].abs())).clamp(min=0)  # (what is left beside the bf16 rounding of the output)
            rest = torch.arange(M, device=DEV) != 77
            Xd = X.double()
            sds = (Xd.mean(1) / Xd.std(1)).abs()
            row = (off, "split + reduce (two-pass)" if split else "fused (one-pass)", float(sds[rest].mean()), float(f32[rest].max()),
                   float(ratio[rest].max()), float(sds[77]), float(f32[77].max()), float(ratio[77].max()))
            OFFSETS.append(row)
            print(OFFSET_FMT % row)
            ratio = float(ratio.max())
            assert ratio <= 1, (off, split, ratio)


# ------------------------------------------------------------------------------------------------ prefix property
@pytest.mark.parametrize("kind", ["plain", "qkv", "split"])
def test_first_rows_do_not_depend_on_the_row_count(lib, kind):
    """The first 129 rows of an M = 300 launch are bit for bit the M = 129 launch (a row depends on itself only; the ragged tile of
    the short launch computes what the full tile of the long one does)."""
    regime = "random"
    prm, dev = params(regime)
    outs = {}
    O, src = R.make_rows(regime, 300, 300, DEV, 9)
    for M in (300, 129):
        c = case(f"prefix_{kind}_{M}", {"plain": 0, "qkv": 1, "split": 3}[kind], M, {"plain": "XH", "qkv": "XQ", "split": "X"}[kind],
                 red="A" if kind == "split" else None)
        L = layout(c)
        _, _, _, bufs = build(c, regime, 0, rows=(O[:M], src[:M]))
        launch(lib, c, L, bufs, dev)
        if kind == "split":
            outs[M] = [bufs["X"][:4 * M].view(4, M, D)[:, :129], bufs["redH"][:129]]
        else:
            outs[M] = [bufs["X"][:129], bufs["H" if kind == "plain" else "Q"][:129]]
    for a, b in zip(outs[300], outs[129]):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(_bits(a), _bits(b))


def test_every_block_form_has_a_case():
    """The cases name exactly the forms of include/m3pc_hip_debug.h (each case asserts that the launcher picked its form).  Prints the
    largest err / bound per (form, stage) seen in the random regime, and the row-offset table."""
    want = header_forms()
    assert want == {0, 1, 2, 3, 16, 17}, sorted(want)
    have = {c["form"] for c in CASES}
    assert have == want, (sorted(want - have), sorted(have - want))
    if WORST:
        print(f"\nfirst / second runs that were exact: {EXACT[0]}")
        print("largest err / bound per (form, stage), random regime:")
        for form in sorted({k for k, _ in WORST}, key=str):
            print(f"  form {form!s:>2}: " + "  ".join(f"{st} {v:.3g}" for (f, st), v in sorted(WORST.items(), key=str) if f == form))
    for o in OFFSETS:
        print(OFFSET_FMT % o)
