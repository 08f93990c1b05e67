"""Float64 restatement of the library's attention (m3pc_debug_attention, include/m3pc_hip_debug.h) and an element-wise bound on
what the fp32 and bf16 kernels may differ from it.

What the hook computes, for batch element b, head h (columns [h hd, (h + 1) hd) of every row) and query slot i:

    keys j over the union, in this order: own rows K1[b] (L1), batch-shared K2 (L2), the pre-reduced block Kp (Lp)
    s_ij = scale * q_i . k_j,    p_ij = exp(s_ij - max_j s_ij) / sum_j exp(...),    O_i = sum_j p_ij v_j

The queries are Q[b] (or Q[0] when the batch shares them), Lq rows, output rows orow1 + i; then the optional batch-shared Q2
(Lq2 rows, output rows orow2 + i).  The kernels' query-slot layout (Q2's slots start at the next multiple of 32 after Lq) does not
change the result and is not modelled.

The bound, per output element (i, h, d), with p_ij the float64 weights, A_ij = scale * sum_d |q_id| |k_jd| (>= |s_ij|),
Amax_i = max_j A_ij, S_id = sum_j p_ij |v_jd| (>= |O_id|) and u = 2^-24 (fp32 unit roundoff):

  fp32 kernels:  E32 = u * (2 Lk + 8 + (2 hd + 8) Amax_i) * S_id
     * a score is an fp32 sum of hd exact products (MFMA f32 or fmaf): error <= hd u A_ij, plus u |s| for the scale;
       s - m and its exponential (expf / exp2 of (s - m) log2 e): relative error of the weight <= 2 u A + 4 u
       (the error of m itself is common to every key and cancels in the normalisation; the split / pair kernels' merge
       factors exp(m_w - m) are of the same kind).  A relative error eps_j of weight j moves O by
       sum_j p_j (eps_j - eps_bar) v_j = sum_j p_j eps_j (v_j - O), at most max|eps| * 2 S: the (2 hd + 8) Amax term;
     * the fp32 sum l of Lk weights, 1 / l and the product with it: (Lk + 2) u relative on all of O (|O| <= S);
     * P V, an fp32 sum of Lk products: Lk u S.
     The pre-reduced block (prestats kernel, fp32 fmaf chains over Lp keys) is counted in Lk.
  bf16 kernels:  E16 = 2^-8 (|O_ref| + S) + (1 + 2^-8) E32
     P is normalised in fp32 and then rounded to bf16 (relative 2^-8 per weight, NOT renormalised: 2^-8 S), and O is rounded
     to bf16 at the store (2^-8 |O_fp32| <= 2^-8 (|O_ref| + E32)).  Scores and sums are fp32 as above (bf16 products are
     exact in fp32).  The pre-reduced block's part of O stays fp32, so 2^-8 S over-counts there.

The bound is a worst case, not a probabilistic one: the sums of the kernels are ~sqrt(n) random walks, so the typical ratio
err / bound sits well below 1 and never depends on luck.  It is tight enough that a dropped key, a V row taken from the wrong side
of a 32-key tile seam, a wrong pre-block merge or an output row shifted by one exceed it (tests/test_attention_ref_cpu.py).
"""
import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8


def _heads(x, n_head):
    return x.reshape(*x.shape[:-1], n_head, x.shape[-1] // n_head)


def attention_ref(q, k1, v1, n_head, scale, q2=None, k2=None, v2=None, kp=None, vp=None, orow1=0, orow2=0, n_rows=None,
                  mutate=None):
    """q (Bq, Lq, W) with Bq 1 (batch-shared) or B; k1 / v1 (B, L1, W); q2 (Lq2, W); k2 / v2 (L2, W); kp / vp (Lp, W); W = n_head hd.
    Any float dtype, on any device; computed in float64 there.  Returns a dict with O (B, R, W) at the output rows (zero elsewhere),
    S = sum_j p |v|, Amax (per element), rows (R,) bool: the rows the call writes, Lk, hd, p (B, n_head, Lq + Lq2, Lk).
    mutate (the bound's own test): ("drop", j) removes key j, ("swap_v", j1, j2) pairs the scores of keys j1 / j2 with each
    other's V rows."""
    f = lambda t: None if t is None else t.to(torch.float64)
    q, k1, v1, q2, k2, v2, kp, vp = map(f, (q, k1, v1, q2, k2, v2, kp, vp))
    B, L1, W = k1.shape
    hd = W // n_head
    Lq = q.shape[1]
    Lq2 = 0 if q2 is None else q2.shape[0]
    keys, vals = [k1], [v1]
    for k, v in ((k2, v2), (kp, vp)):
        if k is not None and k.shape[0]:
            keys.append(k.unsqueeze(0).expand(B, -1, -1))
            vals.append(v.unsqueeze(0).expand(B, -1, -1))
    K, V = torch.cat(keys, 1), torch.cat(vals, 1)
    Lk = K.shape[1]
    Qs = q.expand(B, -1, -1)
    if Lq2:
        Qs = torch.cat([Qs, q2.unsqueeze(0).expand(B, -1, -1)], 1)
    Qh, Kh, Vh = _heads(Qs, n_head), _heads(K, n_head), _heads(V, n_head)  # (B, n, H, hd)
    s = torch.einsum("bihd,bjhd->bhij", Qh, Kh) * scale
    Vu = Vh
    if mutate is not None and mutate[0] == "drop":
        s[..., mutate[1]] = -float("inf")
    elif mutate is not None and mutate[0] == "swap_v":
        perm = torch.arange(Lk, device=K.device)
        perm[mutate[1]], perm[mutate[2]] = mutate[2], mutate[1]
        Vu = Vh[:, perm]
    p = torch.softmax(s, -1)
    O = torch.einsum("bhij,bjhd->bihd", p, Vu).reshape(B, -1, W)
    S = torch.einsum("bhij,bjhd->bihd", p, Vu.abs()).reshape(B, -1, W)
    A = torch.einsum("bihd,bjhd->bhij", Qh.abs(), Kh.abs()) * abs(scale)
    Amax = A.amax(-1).transpose(1, 2).unsqueeze(-1).expand(B, -1, n_head, hd).reshape(B, -1, W)
    R = n_rows if n_rows is not None else max(orow1 + Lq, orow2 + Lq2)
    out = {"O": O.new_zeros(B, R, W), "S": O.new_zeros(B, R, W), "Amax": O.new_zeros(B, R, W),
           "rows": torch.zeros(R, dtype=torch.bool, device=O.device), "Lk": Lk, "hd": hd, "p": p}
    for r0, a, n in ((orow1, 0, Lq), (orow2, Lq, Lq2)):
        if n:
            for key, t in (("O", O), ("S", S), ("Amax", Amax)):
                out[key][:, r0:r0 + n] = t[:, a:a + n]
            out["rows"][r0:r0 + n] = True
    return out


def bound(ref, dtype):
    """Element-wise bound (B, R, W) on |O_kernel - O_ref| for dtype 0 (fp32 kernels) or 1 (bf16 kernels); see the module docstring."""
    Lk, hd = ref["Lk"], ref["hd"]
    e32 = U32 * (2 * Lk + 8 + (2 * hd + 8) * ref["Amax"]) * ref["S"]
    if dtype == 0:
        return e32
    return U16 * (ref["O"].abs() + ref["S"]) + (1 + U16) * e32


REGIMES = ("randn", "peaked", "offset", "same")


def make_inputs(regime, B, Lq, L1, n_head, hd, Lq2=0, L2=0, Lp=0, shared_q=False, dom=None, dtype=1, device="cpu", seed=0):
    """Logical inputs of one case (float32 tensors holding the values the kernel sees: bf16-rounded for dtype 1), shapes as
    attention_ref takes them.  Score regimes (scale = hd^-1/2):
      randn:  every element N(0, 1): scores ~ N(0, 1);
      peaked: q = +-(1, .., 1) + 0.3 N (a random sign per query row), keys 8 N: scores ~ N(0, 8.4^2) (spread +-30); key `dom`
              (index over own, shared, pre keys; default the last) is +60 hd^-1/2 (1, .., 1) + 0.1 N and a second key (index 0, or
              the last when dom is 0) the same with -60: every query gives >= 0.9 of its weight to one of the two, by its sign --
              the rows of a batch element differ, so a misplaced output row shows;
      offset: q = 1 + 0.5 N, every key N + 300 hd^-1/2 (1, .., 1): a common score offset of 200..400 per query;
      same:   every key row (own, shared, pre) one vector: uniform weights."""
    g = torch.Generator(device=device).manual_seed(seed)
    W = n_head * hd
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    Lk = L1 + L2 + Lp
    if regime == "randn":
        qs = lambda *s: rn(*s)
        ks = lambda *s: rn(*s)
    elif regime == "peaked":
        qs = lambda *s: torch.sign(rn(*s[:-1], 1)) + 0.3 * rn(*s)
        ks = lambda *s: 8 * rn(*s)
    elif regime == "offset":
        qs = lambda *s: 1 + 0.5 * rn(*s)
        ks = lambda *s: rn(*s) + 300 / hd ** 0.5
    elif regime == "same":
        qs = lambda *s: rn(*s)
        one = rn(W)
        ks = lambda *s: one.expand(*s).clone()
    else:
        raise ValueError(regime)
    t = {"q": qs(1 if shared_q else B, Lq, W), "k1": ks(B, L1, W), "v1": rn(B, L1, W),
         "q2": qs(Lq2, W) if Lq2 else None, "k2": ks(L2, W) if L2 else None, "v2": rn(L2, W) if L2 else None,
         "kp": ks(Lp, W) if Lp else None, "vp": rn(Lp, W) if Lp else None}
    if regime == "peaked":
        j = Lk - 1 if dom is None else dom
        for jj, sg in ((j, 1.0), (0 if j else Lk - 1, -1.0)):
            if jj == j and sg < 0:  # (a single key)
                continue
            hot = lambda *s: sg * 60 / hd ** 0.5 + 0.1 * rn(*s)
            if jj < L1:
                t["k1"][:, jj] = hot(B, W)
            elif jj < L1 + L2:
                t["k2"][jj - L1] = hot(W)
            else:
                t["kp"][jj - L1 - L2] = hot(W)
    if dtype == 1:
        t = {k: None if v is None else v.to(torch.bfloat16).float() for k, v in t.items()}
    return t
