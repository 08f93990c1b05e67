"""Environments that step together (``HipPlanner.action_sample_batch(lockstep=True)``): ONE policy pass at batch E
(m3pc_policy_pass_batch), every window's own candidate pass back to back, ONE fp32 re-score pass over all windows' re-score
sets (m3pc_score_actions) and one host read of all certificates -- the fp32 chains are paid once per call instead of once
per window.  ``lockstep="native"`` runs the same protocol as ONE library call per group of windows (m3pc_plan_steps_certified,
``_native_group``): per window the bits of the Python path.  A mixin of ``HipPlanner``; the certificate protocol itself is
m3pc_amd/certificate.py."""
from __future__ import annotations

import types
import warnings

import numpy as np
import torch

from . import capi
from .certificate import _WindowOps, resolve as _resolve_certificate

_MODES = {"rtg_guiding": capi.MODE_RTG, "critic_lambda_guiding": capi.MODE_CRITIC, "noise_adding_lambda": capi.MODE_NOISE}


class LockstepMixin:
    def _action_sample_lockstep(self, sequence_histories, percentage=1.0, eval=False, rtg=None, onepass: bool = False,
                                native: bool = False, store=None, env_ids=None):
        if native and self.precision in capi.LOW_PRECISION and self.rescore != "bound":
            # (the call runs the certificate protocol on a low-precision pass; rescore="topk" / "none" select differently)
            raise ValueError(f"lockstep='native' runs the certified re-score (rescore='bound') behind a low-precision candidate pass; "
                             f"rescore={self.rescore!r} is served by lockstep=True")
        self._drain()
        cfg = self.cfg
        guidance = cfg.plan_guidance
        assert guidance in _MODES, guidance
        mode = _MODES[guidance]
        lmbda = 0.6 if guidance == "rtg_guiding" else float(cfg.lmbda)  # learner.py:405-407
        T, S, A, N = self.T, self.S, self.A, int(cfg.action_samples)
        win = None
        if store is not None:
            # the windows come from the episode store (m3pc_episodes_windows: assembled on the device, the bits of _window_host),
            # the horizons from its mirror of the path lengths
            win = store.windows(env_ids, horizon=int(cfg.horizon), mode="plan")
        E = len(sequence_histories) if win is None else win[0].shape[0]
        rtgs = [rtg] * E if (rtg is None or np.isscalar(rtg)) else list(rtg)
        if eval:
            assert all(r is not None for r in rtgs)
        if win is None:
            host = np.empty((E, T * (S + A + 1)), dtype=np.float32)
            meta = []
            for i, hst in enumerate(sequence_histories):
                meta.append(self._window_host(hst, rtgs[i], percentage, host[i]))
            dev = torch.from_numpy(host).to(self.device)  # one packed H2D copy for all windows
        else:
            meta = [(int(h), self._rtg_value(rtgs[i], percentage)) for i, h in enumerate(win[3])]
        out = torch.empty((E, A), dtype=torch.float32, device=self.device)
        info = [None] * E
        groups = []
        for h in sorted({m[0] for m in meta}):  # windows of one effective horizon, at most max_batch of them per group
            same = [i for i, m in enumerate(meta) if m[0] == h]
            groups += [(h, same[c0 : c0 + self._max_batch]) for c0 in range(0, len(same), self._max_batch)]
        for h, ids in groups:
            if win is None:
                sel = dev if len(ids) == E else dev[torch.tensor(ids, device=self.device)]
                s = sel[:, : T * S].reshape(-1, T, S).contiguous()
                a = sel[:, T * S : T * (S + A)].reshape(-1, T, A).contiguous()
                r = sel[:, T * (S + A) :].reshape(-1, T, 1).contiguous()
            else:
                s, a, r = win[:3] if len(ids) == E else [x[torch.tensor(ids, device=self.device)] for x in win[:3]]
            Eg = len(ids)
            eps = self._eps((Eg, N, h, A)) if mode == capi.MODE_NOISE else self._eps((Eg, N, T, A))
            # lockstep="native": the whole group in ONE library call (m3pc_plan_steps_certified).  While the weight load's
            # calibration windows are not used up the group takes the Python path below -- that path is what calibrates
            calibrating = self.rescore == "bound" and self._delta_fixed is None and (self._delta0 is None or self._cal_left > 0)
            if native and calibrating and self._eval_tol is not None:
                # (the eval_action certificate has no Python form to fall back to: calibrate on the group's own passes, then the call)
                self._calibrate_group(mode, s, a, r, [meta[i][1] for i in ids], eps, h, lmbda)
                calibrating = False
            if native and not calibrating:
                self._native_group(mode, s, a, r, [meta[i][1] for i in ids], eps, h, lmbda, ids, eval, out, info)
                continue
            if onepass:
                res = self.handle.plan_step_batch(mode, s, a, r, [meta[i][1] for i in ids], eps, h, lmbda, float(cfg.discount), N,
                                                  precision=self.precision)
            else:
                # ONE policy pass at batch Eg, then every window's own candidate pass (first-layer history sharing and the two
                # candidate halves as in the single-window step), back to back: the caller's stream joins the halves once, at the end
                f32 = dict(dtype=torch.float32, device=self.device)
                res = dict(expect_return=torch.empty((Eg, N), **f32), sample_actions=torch.empty((Eg, N, h, A), **f32),
                           loc=torch.empty((Eg, T, A), **f32), std=torch.empty((Eg, T, A), **f32))
                self.handle.policy_pass_batch(mode, s, a, r, h, [meta[i][1] for i in ids], slot=0)
                for w in range(Eg):
                    self.handle.candidate_pass(mode, s[w], a[w], r[w], eps[w], h, lmbda, float(cfg.discount), N, precision=self.precision,
                                               slot=0, window=w, defer_join=True,
                                               out={k: v[w] for k, v in res.items()})
                self.handle.candidate_join(0)
            er, acts = res["expect_return"], res["sample_actions"]
            stats_h = None
            merged = [er[w] for w in range(Eg)]
            # the multinomial's exponentials of every window (the same order of draws as before the race lists needed them early)
            expos = [torch.empty((N,), dtype=torch.float32, device=self.device).exponential_(1, generator=self.generator)
                     for _ in range(Eg)]
            temp = float(cfg.temperature)
            bound = self.rescore == "bound"
            if self.rescore != "none":
                smode = capi.MODE_RTG if mode == capi.MODE_RTG else capi.MODE_CRITIC
                R = self._R if bound else 0
                if bound:
                    if self._delta_fixed is None and (self._delta0 is None or self._cal_left > 0):
                        # calibrate on this group's windows -- all of a window's candidates in fp32 -- until the weight load's
                        # calibration windows are used up (round 6: the same count as the single-window steps take, certificate
                        # sweeps of DESIGN section 5; round 5 took window 0 of the first group only)
                        d0 = self._delta0 or 0.0
                        n_cal = max(1, min(Eg, self._cal_left))
                        for w in range(n_cal):
                            f32 = self.handle.score_actions(smode, s[w], a[w], r[w], acts[w], None, h, lmbda, float(cfg.discount))
                            d = er[w] - f32
                            d0 = max(d0, self.calibration_factor * float((d - d.median()).abs().max()), 1e-6 * float(f32.abs().max()), 1e-30)
                        self._delta0 = d0
                        self._cal_left = max(0, self._cal_left - n_cal)
                    # The certified re-score of certificate.py, for all windows of the group at once: the kmin best candidates
                    # by score and the rfirst best by race key of every window in ONE fp32 pass, merge + select enqueued for
                    # every window, THEN one host read of the certificates; windows that ask for more get passes of their own.
                    kmax = max(min(self.rescore_max, N - 1 if N > 1 else 1, 1024 - self._R - 1), 1)  # (merge kernels: r + n <= 1024)
                    rfirst = max(min(self.race_min, R), 1) if R > 0 else 0
                    kmin = max(min(self.rescore_min - rfirst, N, kmax), 1)  # (the race entries share the floor of the first pass)
                    lsts, blst = [], []
                    for w in range(Eg):
                        bt = torch.empty((R + kmax + 1,), dtype=torch.float32, device=self.device)
                        if R > 0:
                            lsts.append(self.handle.topk_race_window(er[w], expos[w], temp, kmax, kmin, R, list_scores=bt)[0])
                        else:
                            lsts.append(self.handle.topk_window(er[w], kmax, kmin, 0.0, top_scores=bt)[0])
                        blst.append(bt)
                else:
                    kmax = kmin = min(self.rescore_topk, N)
                    rfirst = 0
                    lsts = [torch.topk(er[w], kmin).indices.to(torch.int32) for w in range(Eg)]
                    blst = [er[w][lsts[w].long()].contiguous() for w in range(Eg)]
                delta = float(self._delta) if bound else 0.0
                m0 = rfirst + kmin
                pick = torch.cat([lsts[w][R - rfirst : R + kmin].long() for w in range(Eg)])
                wsel = torch.arange(Eg, dtype=torch.int32, device=self.device).repeat_interleave(m0)
                f32 = self.handle.score_actions(smode, s, a, r, acts[wsel.long(), pick], wsel, h, lmbda, float(cfg.discount))
                flst, mstats = [], []
                for w in range(Eg):  # fp32 scores for the sets, shift-corrected bf16 scores for the rest (m3pc_rescore_merge[_race])
                    fl = torch.empty_like(blst[w])
                    fl[R - rfirst : R + kmin] = f32[w * m0 : (w + 1) * m0]
                    flst.append(fl)
                    o = R - rfirst
                    if bound and R > 0:
                        merged[w], st_w = self.handle.rescore_merge_race(er[w], expos[w], temp, lsts[w][o:], rfirst, kmin, blst[w][o:],
                                                                        fl[o:], delta=delta)
                    else:
                        merged[w], st_w = self.handle.rescore_merge(er[w], lsts[w], kmin, blst[w], fl, delta=delta)
                    mstats.append(st_w)
            sels = [self.handle.select(merged[j], acts[j, :, 0], temp, expos[j]) for j in range(Eg)]
            certs = [None] * Eg
            counts = [kmin if self.rescore != "none" else 0] * Eg
            if bound:
                stats_h = torch.stack(mstats).cpu()  # the one host read of the group: the certificates' statistics per window
                ctx = types.SimpleNamespace(hdl=self.handle, cap=max(self.handle.max_rescore, 1), disc=float(cfg.discount),
                                            temp=temp, stats_h=stats_h, smode=smode, s=s, a=a, r=r, acts=acts, h=h,
                                            lmbda=lmbda, N=N, er=er, lsts=lsts, blst=blst, flst=flst, merged=merged, sels=sels,
                                            expos=expos, R=R, wset=[None] * Eg, nd=[kmin] * Eg, rd=[rfirst] * Eg)
                delta_first = delta
                for w in range(Eg):
                    ops_w = _WindowOps(ctx, w)
                    if delta > delta_first:  # an earlier window of the group raised the bound: this window's certificate again, under it
                        ops_w.merge_select(ctx.nd[w], ctx.rd[w], delta)
                    certs[w] = _resolve_certificate(self, N, kmax, R, ctx.nd[w], ctx.rd[w], delta, ops_w)
                    if certs[w]["delta"] > delta:  # this window saw a larger deviation than the bound: raised for everybody from here on
                        delta = certs[w]["delta"]
                        self._delta0 = max(self._delta0, delta)  # (the base bound, not the setter: calibration windows still to come stay)
                    counts[w] = certs[w]["n_rescored"]
            for j, i in enumerate(ids):
                p, ev, am, si, sa = sels[j]
                out[i] = ev if eval else sa[0]
                info[i] = dict(expect_return=merged[j], argmax=am, sample_idx=si, eval_action=ev, sample_action=sa, horizon=h,
                               n_rescored=None if certs[j] is None else counts[j],
                               n_race=None if certs[j] is None else certs[j]["n_race"],
                               min_margin_outside=None if certs[j] is None else certs[j]["min_margin_outside"],
                               saturated=None if certs[j] is None else certs[j]["saturated"],
                               delta=self._delta)
        self._mark_main()
        self.last = dict(windows=info, delta=self._delta)
        return out

    def _calibrate_group(self, mode, s, a, r, rtgs, eps, h, lmbda):
        """The calibration of the Python path on a group's windows, alone: the group's policy pass and candidate passes in the
        planner's precision, every candidate of the first windows in fp32, the bound folded into ``_delta0``.  No variate is drawn."""
        cfg = self.cfg
        Eg, N, T, A = s.shape[0], int(cfg.action_samples), self.T, self.A
        f32 = dict(dtype=torch.float32, device=self.device)
        res = dict(expect_return=torch.empty((Eg, N), **f32), sample_actions=torch.empty((Eg, N, h, A), **f32),
                   loc=torch.empty((Eg, T, A), **f32), std=torch.empty((Eg, T, A), **f32))
        self.handle.policy_pass_batch(mode, s, a, r, h, rtgs, slot=0)
        n_cal = max(1, min(Eg, self._cal_left))
        for w in range(n_cal):
            self.handle.candidate_pass(mode, s[w], a[w], r[w], eps[w], h, lmbda, float(cfg.discount), N, precision=self.precision,
                                       slot=0, window=w, defer_join=True, out={k: v[w] for k, v in res.items()})
        self.handle.candidate_join(0)
        smode = capi.MODE_RTG if mode == capi.MODE_RTG else capi.MODE_CRITIC
        d0 = self._delta0 or 0.0
        for w in range(n_cal):
            er = res["expect_return"][w]
            f = self.handle.score_actions(smode, s[w], a[w], r[w], res["sample_actions"][w], None, h, lmbda, float(cfg.discount))
            d = er - f
            d0 = max(d0, self.calibration_factor * float((d - d.median()).abs().max()), 1e-6 * float(f.abs().max()), 1e-30)
        self._delta0 = d0
        self._cal_left = max(0, self._cal_left - n_cal)

    def _native_group(self, mode, s, a, r, rtgs, eps, h, lmbda, ids, eval, out, info):
        """One group of a lock-step batch through m3pc_plan_steps_certified: the draws, the first-pass sizes and the bound are
        those of the Python path above; ``info`` and the bound are filled from the windows' records.  Two things are the
        records' and not the Python path's: ``delta_grown`` counts the WINDOWS that came out with a larger bound (``resolve``
        counts every raise, and a window may raise more than once), and the bound folded back into ``_delta0`` is
        ``records[-1].delta``, the float the ABI carries, where the Python path keeps the double 1.5 x deviation -- the same
        number after one rounding to float, which is what every kernel is given."""
        cfg = self.cfg
        Eg, N = len(ids), int(cfg.action_samples)
        # the multinomial's exponentials, window by window: the generator is consumed exactly as by the Python path
        expo = torch.empty((Eg, N), dtype=torch.float32, device=self.device)
        for w in range(Eg):
            expo[w].exponential_(1, generator=self.generator)
        bound = self.rescore == "bound"
        R = self._R if bound else 0
        kmin = kmax = 1
        rfirst, delta = 0, 0.0
        if bound:
            kmax = max(min(self.rescore_max, N - 1 if N > 1 else 1, 1024 - self._R - 1), 1)
            rfirst = max(min(self.race_min, R), 1) if R > 0 else 0
            kmin = max(min(self.rescore_min - rfirst, N, kmax), 1)
            delta = float(self._delta)
        got = self.handle.plan_steps_certified(mode, s, a, r, rtgs, eps, expo, h, lmbda, float(cfg.discount), N,
                                               float(cfg.temperature), delta=delta,
                                               grow_delta=bound and self._delta_fixed is None, kmin=kmin, kmax=kmax,
                                               rfirst=rfirst, rmax=R, precision=self.precision, slot=0, want_policy=False,
                                               want_list=False, want_p=False, eval_tol=self._eval_tol)
        res, recs = got[0], got[1]
        erecs = got[2] if len(got) > 2 else None  # (eval_tol: m3pc_plan_steps_certified_eval)
        if bound:
            seen = float(np.float32(delta))
            for rec in recs:  # (a window that raised the bound raised it for every later window of the group)
                if rec.delta > seen:
                    seen = float(rec.delta)
                    self.delta_grown += 1
            if seen > float(np.float32(delta)):
                self._delta0 = max(self._delta0, float(recs[-1].delta))
            if any(rec.saturated for rec in recs) and not self._warned_saturated:
                self._warned_saturated = True
                warnings.warn(f"m3pc_amd: the certificates of a lock-step window asked for more candidates than it lists "
                              f"(delta={recs[-1].delta:.3g}, rescore_max={self.rescore_max}); the whole window set or every candidate "
                              f"was re-scored in fp32 (slow path)")
        _, ev, am, si, sa = res["sel"]
        for j, i in enumerate(ids):
            out[i] = ev[j] if eval else sa[j]
            rec = recs[j] if bound else None
            info[i] = dict(expect_return=res["expect_return"][j], argmax=am[j : j + 1], sample_idx=si[j : j + 1], eval_action=ev[j],
                           sample_action=sa[j : j + 1], horizon=h,
                           n_rescored=None if rec is None else int(rec.n_rescored), n_race=None if rec is None else int(rec.n_race),
                           min_margin_outside=None if rec is None else float(rec.margin),
                           saturated=None if rec is None else bool(rec.saturated), delta=self._delta)
            if erecs is not None:
                e = erecs[j]
                info[i].update(eval_bound=float(e.eval_bound), need_eval_first=int(e.need_eval_first), n_eval=int(e.n_eval),
                               eval_rounds=int(e.eval_rounds), eval_certified=bool(e.eval_certified),
                               everything=bool(recs[j].everything))

