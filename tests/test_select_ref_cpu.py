"""CPU checks behind tests/test_select_edges_gpu.py: the references of tests/select_ref.py against torch in float64 (softmax, topk,
median) and against the oracle's select; every bound against a float32 NumPy evaluation of its own operation; every refusal of the new
hooks on fake pointers (a refusal comes before anything is launched, so no GPU is needed); the case table against the header's kernel
ids; and, for every case of the GPU file, that its inputs leave NO decision inside a rounding bound -- zero cases excused -- so that
the GPU file may compare lists and counts for equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import select_ref as R
import test_select_edges_gpu as G

F = np.float32


# ------------------------------------------------------------------------------------------------ references against torch
@pytest.mark.parametrize("regime", R.TOPK_REGIMES)
@pytest.mark.parametrize("n", [1, 65, 2049])
def test_topk_order_is_torchs_stable_sort(regime, n):
    v = R.topk_values(regime, n, n)
    want = torch.sort(-(torch.from_numpy(v).double() + 0.0), stable=True).indices.numpy()
    assert np.array_equal(R.topk_order(v), want)
    k = min(n, 17)
    if regime == "randn":  # (distinct values: torch.topk has no tie rule to differ by)
        assert np.array_equal(R.topk_order(v, k), torch.topk(torch.from_numpy(v).double(), k).indices.numpy())
    z = np.array([0.0, -0.0, 1.0, -0.0, 0.0], F)
    assert R.topk_order(z).tolist() == [2, 0, 1, 3, 4]


@pytest.mark.parametrize("n,regime", [(1, "tau1"), (65, "tau0.01"), (1025, "tau1"), (5000, "tau0.01")])
def test_select_ref_is_torchs_softmax_and_the_oracles_select(n, regime):
    from oracle import mtm_oracle as O
    e, a0, tau, q = R.select_inputs(regime, n, 3, n)
    p, ev, am, si = R.select_ref(e, a0, tau, q)
    t = torch.from_numpy(e).double()
    pt = torch.softmax(float(F(tau)) * (t - t.max()), 0)
    assert np.abs(p - pt.numpy()).max() <= 1e-15 and am == int(torch.argmax(t)) and si == int(torch.argmax(pt / torch.from_numpy(q).double()))
    assert np.abs(ev - (pt[:, None] * torch.from_numpy(a0).double()).sum(0).numpy()).max() <= 1e-14
    pr, evr = O.select(O.PlanCfg(8, 4, n, temperature=tau), torch.from_numpy(e), torch.from_numpy(a0))
    assert np.abs(p - pr.double().numpy().reshape(-1)).max() <= 1e-5 and np.abs(ev - evr.double().numpy().reshape(-1)).max() <= 1e-5


@pytest.mark.parametrize("m", [1, 2, 3, 8, 1024, 1025])
def test_lower_median_is_torch_median(m):
    d = np.round(R.rng(m).standard_normal(m) * 4).astype(F)  # (ties)
    assert R.lower_median(d) == float(torch.from_numpy(d).double().median()) == np.sort(d)[(m - 1) // 2]
    b, f = G.calib_case(max(m, 8))
    c, dev, fmx = R.deviation_ref(b, f)
    dd = torch.from_numpy(b) - torch.from_numpy(f)
    assert c == float(dd.median()) and dev == float((dd - dd.median()).abs().max()) and fmx == float(torch.from_numpy(f).abs().max())


# ------------------------------------------------------------------------------------------------ bounds against float32 NumPy
@pytest.mark.parametrize("n", [1, 2, 65, 1025, 16385])
@pytest.mark.parametrize("regime", ["tau0.01", "tau1"])
def test_select_bounds_hold_for_a_float32_evaluation(n, regime):
    e, a0, tau, q = R.select_inputs(regime, n, 17, n)
    p64, ev64, _, _ = R.select_ref(e, a0, tau)
    p32, ev32 = R.select_ref32(e, a0, tau)
    bp, be = R.select_p_bound(e, tau), R.select_eval_bound(e, a0, tau)
    assert (np.abs(p32 - p64) <= bp).all(), float((np.abs(p32 - p64) / bp).max())
    assert (np.abs(ev32 - ev64) <= be).all(), float((np.abs(ev32 - ev64) / be).max())
    assert (bp <= 1e-4 * p64 + 2 * R.TINY).all() and (be <= 1e-4 * (np.abs(a0).T @ p64) + 1e-30).all()  # (a bound, not a tolerance)


@pytest.mark.parametrize("n,flavour", [(65, "tau0.01"), (2049, "tau1"), (16384, "tau0.01")])
def test_key_bound_holds_for_a_float32_evaluation(n, flavour):
    e, q, tau, _, _ = G.race_case(n, flavour)
    err = np.abs(R.race_key32(tau, e, q).astype(np.float64) - R.race_keys64(tau, e, q))
    b = R.key_bound(tau, e, q)
    assert (err <= b).all() and (b <= 2e-6 * (np.abs(R.race_keys64(tau, e, q)) + np.abs(np.log(q.astype(np.float64))) + 5.0)).all()


def test_restatements_on_hand_made_inputs():
    v = np.array([5.0, 1.0, 5.0, 3.0, 4.5, 4.0], F)
    idx = R.topk_order(v, 4)
    assert idx.tolist() == [0, 2, 4, 5]
    (n, margin, mx, cnt), top = R.window_stats_ref(v, idx, 4, 1, 3, 0.5, 1, np.array([3], np.int32))
    assert (n, float(margin), float(mx), cnt) == (3, 1.0, 5.0, 3) and top.tolist() == [3.0, 5.0, 5.0, 4.5, 4.0]
    assert R.window_stats_ref(v, idx, 4, 1, 8, 9.0)[0][:2] == (4, F(np.inf))
    b = np.array([10.0, 9.0, 8.0, 7.0, 9.0], F)
    lst = np.array([3, 0, 1], np.int32)  # one racer, two score entries
    f = np.array([6.0, 9.5, 8.0], F)
    ref = R.merge_ref(b, lst, 1, 2, b[lst], f, 0.25)
    assert (float(ref["c"]), float(ref["dev"]), ref["need"]) == (1.0, 0.5, 0) and float(ref["thr"]) == 10.25
    assert ref["merged"].tolist() == [9.5, 8.0, 7.0, 6.0, 8.0] and float(ref["margin"]) == 10.25 - 8.0  # (the tie with b_last is not `outside`)
    assert R.scatter_ref(np.zeros(4, F), np.array([1, 2], F), [3, 0]).tolist() == [2.0, 0.0, 0.0, 1.0]


def test_block_sum_emulation_and_the_psum_that_is_not_one():
    """block_sum32 adds what it is given (exactly, on integers), and the underflow25 cases hold a psum other than 1: only there does a
    select that divided eval_action by 1 instead of psum give other bits."""
    x = R.rng(1).integers(-50, 51, 16385).astype(F)
    assert R.block_sum32(R.thread_sums32(x)) == x.astype(np.float64).sum()
    seen = 0
    for n in G.SELECT_SIZES:
        if n < 1023:
            continue
        e, a0, tau, q = G.select_case(n, "underflow25", 3)
        p32, ev32, psum = R.select_underflow32(e, a0)
        t = (ev32.astype(np.float64) * np.float64(psum)).astype(F)
        seen += int(psum != 1.0 and not np.array_equal(F(t / psum), F(t / F(1.0))))
    assert seen >= 3, seen


# ------------------------------------------------------------------------------------------------ refusals, on fake pointers
@pytest.fixture(scope="module")
def lab():
    from hip_util import lab_library
    return G.declare(lab_library())


def test_refusals_come_before_any_launch(lab):
    fake = 0x1000
    st = None
    # m3pc_debug_topk keeps its signature and gains the refusals
    for v, n, k, out in ((None, 8, 1, fake), (fake, 8, 1, None), (fake, 0, 1, fake), (fake, 16385, 1, fake), (fake, 8, 0, fake), (fake, 8, 9, fake)):
        assert lab.m3pc_debug_topk(v, n, k, out, st) == -1, (v, n, k, out)

    def ex(**kw):
        a = G.TopkArgs()
        a.v, a.out, a.n_windows, a.n, a.k, a.out_stride = fake, fake, 1, 4096, 8, 1
        for key, val in kw.items():
            setattr(a, key, val)
        return lab.m3pc_debug_topk_ex(C.byref(a))

    assert lab.m3pc_debug_topk_ex(None) == -1
    bad = [dict(v=None), dict(out=None), dict(n=0), dict(n=16385), dict(k=0), dict(k=4097), dict(n_windows=0), dict(out_stride=2), dict(out_stride=0),
           dict(variant=-1), dict(variant=7), dict(variant=6, expo=fake), dict(variant=6, out_stride=-1), dict(variant=1), dict(variant=2), dict(variant=1, n=2049, k=1), dict(variant=2, n=2049, k=1),
           dict(variant=3, k=65), dict(variant=3, n_windows=2), dict(variant=4, n_windows=2), dict(variant=4, out_stride=-1),
           dict(variant=4, expo=fake), dict(variant=0, out_stride=-1), dict(variant=0, scores_out=fake), dict(variant=0, kk=3),
           dict(variant=5), dict(variant=5, expo=fake, out_stride=-1, kk=0), dict(variant=5, expo=fake, out_stride=1, kk=8),
           dict(variant=5, expo=fake, out_stride=-1, kk=8, scores_out=fake), dict(variant=0, expo=fake, out_stride=-1, kk=4097),
           dict(variant=0, expo=fake, out_stride=-1, kk=1025), dict(variant=0, expo=fake, out_stride=-1, kk=8, k=65),
           dict(variant=0, expo=fake, out_stride=-1, kk=8, n_windows=2), dict(variant=0, expo=fake, out_stride=-1, kk=9, n=8, k=8)]
    for kw in bad:
        assert ex(**kw) == -1, kw
        assert lab.m3pc_last_error()
    ws = lab.m3pc_debug_window_stats
    good = dict(v=fake, n_total=100, idx=fake, kk=10, kmin=1, kmax=9, window=0.0, stats=fake, host=None, seq=0.0, top=None, rr=0)
    for kw in (dict(v=None), dict(idx=None), dict(stats=None), dict(n_total=0), dict(n_total=16385), dict(kk=0), dict(kk=101), dict(kmin=0),
               dict(kmin=10), dict(rr=-1), dict(rr=65), dict(window=-1.0), dict(window=float("nan"))):
        a = dict(good, **kw)
        assert ws(a["v"], a["n_total"], a["idx"], a["kk"], a["kmin"], a["kmax"], a["window"], a["stats"], a["host"], a["seq"], a["top"], a["rr"], st) == -1, kw
    sc = lab.m3pc_debug_scatter
    for src, index, n, dst in ((None, fake, 1, fake), (fake, None, 1, fake), (fake, fake, 1, None), (fake, fake, 0, fake)):
        assert sc(src, index, n, dst, None, st) == -1
    vb = lab.m3pc_debug_variates_batch
    steps = (C.c_ulonglong * 2)(1, 2)
    for stp, E, g0, g1, out in ((None, 2, 0, 8, fake), (steps, 2, 0, 8, None), (steps, 0, 0, 8, fake), (steps, 2, -1, 8, fake), (steps, 2, 8, 8, fake),
                                (steps, 2, 0, (1 << 33) + 1, fake)):
        assert vb(1, stp, E, g0, g1, out, st) == -1
    assert lab.m3pc_debug_select_picked() == 0  # (nothing was launched)


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_names_exactly_the_headers_ids():
    ids = G.header_ids()
    assert len(ids) == 23 and sorted(ids) == list(range(1, 24)), ids
    named = set().union(*G.CASE_IDS.values())
    assert named == set(ids), (sorted(set(ids) - named), sorted(named - set(ids)))
    src = open(G.os.path.join(G.ROOT, "m3pc_amd", "csrc", "select.hip")).read()
    kernels = G.re.findall(r"__global__[^\n]*?void (\w+)\(", src)
    assert sorted(kernels) == sorted(ids.values()), "the header's list is not the __global__ kernels of select.hip"
    picks = {int(i) for i in G.re.findall(r"M3PC_SEL_PICK\((?:one_block \? )?(\d+)", src)} | {7}
    assert picks == set(ids), sorted(picks ^ set(ids))
    # every (n, k) reaches a legal kernel; every size the issue lists appears where its kernel accepts it
    for n in R.SIZES:
        for k in G.topk_ks(n):
            assert {kid for _, kid in G.topk_variants(n, k)} <= G.CASE_IDS["topk"]
    assert {kid for n in R.SIZES for k in G.topk_ks(n) for _, kid in G.topk_variants(n, k)} == G.CASE_IDS["topk"]
    assert {G.topk_batch_kid(n, k) for n in R.SIZES for k in G.topk_batch_ks(n)} == G.CASE_IDS["topk_batch"]


# ------------------------------------------------------------------------------------------------ decisive gaps: zero cases excused
@pytest.mark.parametrize("n,flavour", G.race_cases())
def test_race_lists_are_decided(n, flavour):
    e, q, tau, rr, kk = G.race_case(n, flavour)
    keys, bound = R.race_keys64(tau, e, q), R.key_bound(tau, e, q)
    assert R.close_pairs(keys, bound, rr) == [], "two race keys among the listed positions lie closer than their bounds"
    if flavour == "tie" and n >= 2:
        o = R.topk_order(keys, 2)
        assert keys[o[0]] == keys[o[1]] and e[o[0]] == e[o[1]] and q[o[0]] == q[o[1]] and o[0] < o[1]  # the planted tie, bit-equal inputs


@pytest.mark.parametrize("n", R.SIZES)
def test_race_batch_lists_are_decided(n):
    rmax = min(64, n)
    for w in range(max(G.WINDOWS)):
        e, q, tau, _, _ = G.race_case(n, "tau0.01", seed=w)
        assert R.close_pairs(R.race_keys64(tau, e, q), R.key_bound(tau, e, q), rmax) == [], (n, w)


@pytest.mark.parametrize("n", G.SELECT_SIZES)
def test_select_winners_are_decided(n):
    for (n_, regime, A, mult) in [c for c in G.select_cases() if c[0] == n]:
        e, a0, tau, q = G.select_case(n, regime, A)
        assert not np.isnan(e).any() and (q > 0).all()
        gap, allowed = R.race_ratio_margin(e, tau, q)
        p = R.select_ref(e, None, tau)[0]
        ratio = p / q.astype(np.float64)
        o = R.topk_order(ratio, 3)
        if regime == "tie" and n >= 4:
            assert gap == 0.0 and e[o[0]] == e[o[1]] and q[o[0]] == q[o[1]] and o[0] < o[1], (n, regime, A)  # the planted tie
            assert ratio[o[2]] < 0.5 * ratio[o[0]]
            assert int((e == e.max()).sum()) == 2  # (and a tie at the arg-max)
        else:
            assert gap > 4 * allowed, (n, regime, A, gap, allowed)
        if regime.startswith("underflow"):
            y = float(F(tau)) * (e.astype(np.float64) - e.max())
            assert ((y == 0) | (y < -300)).all()  # expf(x < -150) is exactly 0 with or without denormals
            m = int((y == 0).sum())
            p32, ev32, psum = R.select_underflow32(e, a0)
            assert np.array_equal(p32, np.where(y == 0, F(1.0) / F(m), F(0))) and np.abs(ev32 - R.select_ref(e, a0, tau)[1]).max() <= 1e-6
            if m in (1, 2, 4):
                assert psum == 1.0 and np.array_equal(ev32, a0[y == 0].astype(np.float64).mean(axis=0).astype(F))


@pytest.mark.parametrize("case", G.MERGE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_merge_counts_are_decided(case):
    r, n, nt, flavour = case
    c = G.merge_case(*case)
    assert len(set(c["lst"][r:].tolist())) == n and len(set(c["lst"][:r].tolist())) == r  # (no candidate twice within a part)
    if r:
        assert c["lst"][r] in c["lst"][:r]  # a candidate in both parts
    ref = R.merge_ref(c["b"], c["lst"], r, n, c["ls"], c["f"], c["delta"], c["q"], c["tau"])
    assert R.thr_gap_clear(ref["keys"], ref["thr_r"], ref["thr_r_bound"] + ref["keys_bound"].max()), "a race key lies within its bound of thr_r"
    d = (c["ls"] - c["f"]).astype(F)
    if flavour == "tied" and r + n >= 8:
        assert int((d == ref["c"]).sum()) >= 2  # a tie at the lower median
    if flavour == "planted" and nt - len(set(c["lst"].tolist())) >= 3:
        p = c["planted"]
        assert c["b"][p["at_thr"]] == ref["thr"] and c["b"][p["above_thr"]] == np.nextafter(ref["thr"], F(np.inf))
        assert ref["need"] == int((c["b"] >= ref["thr"]).sum()) - 1  # (`>=` in place of `>` counts one more)
        if "at_b_last" in p:
            assert c["b"][p["at_b_last"]] == c["ls"][-1] and p["at_b_last"] not in c["lst"]
    if (r + n) % 2 == 0 and flavour == "randn" and r + n > 1:
        s = np.sort(d)
        assert s[(r + n - 1) // 2] != s[(r + n) // 2]  # (a median taken at m / 2 is another value)
    if n >= nt:
        assert ref["margin"] == np.inf


def test_the_merge_cases_cover_the_planted_edges():
    planted = [G.merge_case(*c)["planted"] for c in G.MERGE_CASES if c[3] == "planted"]
    assert sum(1 for p in planted if "at_thr" in p) >= 8 and sum(1 for p in planted if "at_b_last" in p) >= 8
    assert {(r, n) for r, n, _, _ in G.MERGE_CASES} == set(G.MERGE_PAIRS)
    assert any(n == nt for _, n, nt, _ in G.MERGE_CASES) and any(G.merge_case(*c)["delta"] == 0.0 for c in G.MERGE_CASES)


@pytest.mark.parametrize("case", G.WINDOW_CASES, ids=lambda c: "-".join(map(str, c)))
def test_window_cases_hit_their_clamps(case):
    n_total, kk, kmin, kmax, flavour, rr = case
    v, front, idx, window = G.window_case(*case)
    (n, margin, mx, cnt), top = R.window_stats_ref(v, idx, kk, kmin, kmax, window, rr, front)
    assert top.size == rr + kk and np.array_equal(top[rr:], v[idx])
    if flavour == "below_kmin":
        assert cnt < kmin and n == kmin
    if flavour == "above_kmax":
        assert cnt > kmax and n == min(kmax, kk)
    if flavour == "above_kk":
        assert cnt > kk and n == kk and margin == np.inf
    if flavour == "zero":
        assert window == 0.0 and cnt == min(3, n_total)
    if flavour == "edge" and n_total >= 8:
        thr = F(mx - F(window))
        assert int((v == thr).sum()) == 3 and int((v == np.nextafter(thr, F(-np.inf))).sum()) == 3
    if kk == n_total:
        assert n <= kk and (margin == np.inf) == (n == kk)
    assert {c[5] for c in G.WINDOW_CASES} == {0, 1, 64} and any(c[1] == c[0] for c in G.WINDOW_CASES)
