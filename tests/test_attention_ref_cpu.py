"""CPU checks of tests/attn_ref.py, the float64 reference and error bound of tests/test_attention_gpu.py: the reference is the
textbook softmax(q k^T scale) v over the union of its key segments, and its bound is tight enough to catch the bugs it is there
for (a dropped key, a V row from the wrong side of a 32-key tile seam, a dropped shared / pre-block key, the dominant key of a
peaked softmax, an output row shifted by one)."""
import pytest
import torch

import attn_ref as R

# (Lq, Lq2, L1, L2, Lp, orow1, orow2, hd, n_head)
CASES = [(5, 0, 17, 0, 0, 0, 0, 32, 2), (7, 3, 20, 29, 0, 3, 0, 64, 2), (33, 0, 49, 0, 11, 2, 0, 32, 2),
         (4, 9, 49, 79, 0, 0, 4, 32, 1), (9, 0, 1, 32, 33, 0, 0, 64, 1), (31, 0, 65, 0, 63, 0, 0, 32, 1),
         (3, 0, 96, 32, 0, 1, 0, 32, 1)]  # (every Lk <= 128)


def _args(t, c):
    Lq, Lq2, L1, L2, Lp, orow1, orow2, hd, nh = c
    return dict(q=t["q"], k1=t["k1"], v1=t["v1"], n_head=nh, scale=hd ** -0.5, q2=t["q2"], k2=t["k2"], v2=t["v2"], kp=t["kp"],
                vp=t["vp"], orow1=orow1, orow2=orow2)


def _make(regime, c, seed, dom=None):
    Lq, Lq2, L1, L2, Lp, orow1, orow2, hd, nh = c
    return R.make_inputs(regime, 3, Lq, L1, nh, hd, Lq2=Lq2, L2=L2, Lp=Lp, shared_q=Lp > 0, dom=dom, seed=seed)


@pytest.mark.parametrize("ci", range(len(CASES)))
@pytest.mark.parametrize("regime", R.REGIMES)
def test_reference_is_the_textbook_softmax(ci, regime):
    c = CASES[ci]
    Lq, Lq2, L1, L2, Lp, orow1, orow2, hd, nh = c
    t = _make(regime, c, ci)
    ref = R.attention_ref(**_args(t, c))
    d = lambda x: x.double()
    for b in range(3):
        keys = [d(t["k1"][b])] + [d(t[k]) for k in ("k2", "kp") if t[k] is not None]
        vals = [d(t["v1"][b])] + [d(t[v]) for v in ("v2", "vp") if t[v] is not None]
        K, V = torch.cat(keys), torch.cat(vals)
        q = d(t["q"][0 if Lp else b])
        for seg, r0 in ((q, orow1), (d(t["q2"]) if Lq2 else None, orow2)):
            if seg is None:
                continue
            want = torch.cat([torch.softmax(seg[:, h * hd:(h + 1) * hd] @ K[:, h * hd:(h + 1) * hd].T * hd ** -0.5, -1)
                              @ V[:, h * hd:(h + 1) * hd] for h in range(nh)], 1)
            assert torch.allclose(ref["O"][b, r0:r0 + seg.shape[0]], want, rtol=1e-12, atol=1e-12)
    assert int(ref["rows"].sum()) == Lq + Lq2
    assert ref["Lk"] == L1 + L2 + Lp
    if regime == "same":  # uniform weights
        assert torch.allclose(ref["p"], torch.full_like(ref["p"], 1.0 / (L1 + L2 + Lp)), rtol=1e-12, atol=0)
    if regime == "offset":  # the common offset the kernels must subtract
        s = torch.einsum("bid,bjd->bij", t["q"][:, :, :hd].double().expand(3, -1, -1), t["k1"][:, :, :hd].double()) * hd ** -0.5
        assert float(s.min()) > 150 and float(s.max()) < 450


@pytest.mark.parametrize("ci", range(len(CASES)))
@pytest.mark.parametrize("regime", ["randn", "peaked"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_bound_catches_the_bugs_it_is_for(ci, regime, dtype):
    """Every mutation of the reference exceeds the bound somewhere (N(0,1) cases with Lk <= 128 and every peaked case).  In the
    peaked regime the dominant key sits on the key the mutation touches (a key of weight 1e-9 can be dropped unseen by any bound)."""
    c = CASES[ci]
    Lq, Lq2, L1, L2, Lp, orow1, orow2, hd, nh = c
    Lk = L1 + L2 + Lp
    muts = [("drop", L1 - 1)]  # the last own key
    if L2:
        muts.append(("drop", L1))  # the first shared key
    if Lp:
        muts.append(("drop", L1 + L2))  # the first pre-block key
    if Lk >= 33:
        muts.append(("swap_v", 31, 32))  # a V row from the other side of the 32-key seam
    muts.append(("shift",))  # the output rows shifted by one (row r holds query r + 1's result)
    for m in muts:
        dom = (m[1] if m[0] != "shift" else Lk - 1) if regime == "peaked" else None
        t = _make(regime, c, 100 + ci, dom=dom)
        args = _args(t, c)
        ref = R.attention_ref(**args)
        bnd = R.bound(ref, dtype)[:, ref["rows"]]
        if regime == "peaked":
            assert float(ref["p"].amax(-1).min()) >= 0.9  # one key carries >= 0.9 of every query's weight
        O = ref["O"][:, ref["rows"]]
        if m[0] == "shift":
            excess = (O[:, 1:] - O[:, :-1]).abs() - bnd[:, :-1]
        else:
            excess = (R.attention_ref(**args, mutate=m)["O"][:, ref["rows"]] - O).abs() - bnd
        assert float(excess.max()) > 0, f"mutation {m} stays within the bound"
