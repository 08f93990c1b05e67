"""The zero-shot goal-reaching calls of the reference (research/zeroshot_omtm/learner.py: action_id_sample 60-149,
action_piid_sample 151-261, action_piid_list_sample 263-370) and the CEM refinement of a plan, as a mixin of
``HipPlanner`` (m3pc_amd/planner.py: the step pipeline; m3pc_amd/certificate.py: the certified re-score).  Everything here runs
on the planner's handle: ``m3pc_goal_step`` (both forwards of one or a few windows, fp32), ``m3pc_goal_step_batch`` (thousands of
windows per call, exactly pruned, BASELINE config 5), ``m3pc_forward`` and ``m3pc_score_actions``."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import capi
from .tokenizers import SquashedNormal


class GoalMixin:
    # ---------------------------------------------------------------------------------------- zero-shot
    def assemble_goal_window(self, sequence_history, rtg=None, percentage=1.0):
        """research/zeroshot_omtm/learner.py:164-223: the history window, with the observation rows of the
        WHOLE window taken from the buffer (future rows are way-points), shortened near the 1000-step end."""
        dev, (horizon, return_to_go) = self._stage_copy(lambda flat: self._goal_window_host(sequence_history, rtg, percentage, flat))
        states, actions, rewards = self._blocks(dev)
        return states, actions, rewards, horizon, return_to_go

    def _goal_window_host(self, sequence_history, rtg, percentage, flat):
        """Host half of ``assemble_goal_window``: fills the flat window buffer and returns (horizon, rtg)."""
        T = self.T
        horizon = int(self.cfg.horizon)
        end_idx = int(sequence_history["path_length"])
        if end_idx + horizon < T:
            horizon = T - end_idx
        smart = T
        if end_idx + horizon > 1000:
            smart = smart - (end_idx + horizon - 1000)
        hl = T - horizon + 1
        flat[:] = 0.0
        bs, ba, br = self._blocks(flat)
        lo = end_idx - hl + 1
        ba[:hl] = sequence_history["actions"][lo : end_idx + 1]
        br[:hl] = np.asarray(sequence_history["rewards"][lo : end_idx + 1]).reshape(hl, 1)
        bs[:hl] = sequence_history["observations"][lo : end_idx + 1]
        bs[:smart] = sequence_history["observations"][lo : lo + T]
        return horizon, self._rtg_value(rtg, percentage)

    def _goal_tokens(self, states, actions, rewards, rtg):
        T = self.T
        ret = torch.full((1, T, 1), rtg, dtype=torch.float64, device=self.device)
        return [self.handle.tokenize(capi.STATES, states[None]), actions[None].contiguous(),
                self.handle.tokenize(capi.REWARDS, rewards[None]), self.handle.tokenize(capi.RETURNS, ret)]

    def _policy_from(self, toks, masks, h, eval):
        from .masks import mask_rows
        mu, sd = self.handle.forward(toks, mask_rows(masks), want=("actions",))["actions"]
        self._mark_main()
        dist_ = SquashedNormal(mu.unsqueeze(2), sd.unsqueeze(2))
        if eval:
            return dist_.mean[0, self.T - h]
        return dist_.sample(eps=self._eps(tuple(dist_.loc.shape)))[0, self.T - h]

    @torch.no_grad()
    def action_id_sample(self, sequence_history, percentage=1.0, horizon=4, plan=True, eval=False, rtg=None):
        """zeroshot learner.py:60-149: one forward under the goal inverse-dynamics mask."""
        if eval:
            assert rtg is not None
        from .masks import create_gid_mask
        s, a, r, h, rtg_v = self.assemble_goal_window(sequence_history, rtg, percentage)
        toks = self._goal_tokens(s, a, r, rtg_v)
        return self._policy_from(toks, create_gid_mask(self.T, "cpu", self.T - h), h, eval)

    @torch.no_grad()
    def action_piid_sample(self, sequence_history, percentage=1.0, horizon=4, plan=True, eval=False, rtg=None):
        """zeroshot learner.py:151-261: path inference (pi mask) -> write the inferred states into the
        window -> inverse dynamics (fid mask) -> action at T-h."""
        if eval:
            assert rtg is not None
        from .masks import create_fid_mask, create_pi_mask, mask_rows
        T = self.T
        s, a, r, h, rtg_v = self.assemble_goal_window(sequence_history, rtg, percentage)
        idx = T - h
        self._drain()  # (m3pc_goal_step runs in the policy workspace: no pipelined plan step may still be using it)
        # both forwards and the hand-over between them in one library call on the raw window (m3pc_goal_step)
        mu, sd, inferred, window = self.handle.goal_step(s[None], a[None], r[None], [rtg_v], mask_rows(create_pi_mask(T, "cpu", idx)),
                                                         mask_rows(create_fid_mask(T, "cpu", idx)), idx)
        self._mark_main()
        self.last = dict(state_inference=inferred, window_states=window[0])
        dist_ = SquashedNormal(mu.unsqueeze(2), sd.unsqueeze(2))
        if eval:
            return dist_.mean[0, idx]
        return dist_.sample(eps=self._eps(tuple(dist_.loc.shape)))[0, idx]

    @torch.no_grad()
    def action_piid_list_sample(self, sequence_history, percentage=1.0, horizon=4, plan=True, eval=False, rtg=None):
        """zeroshot learner.py:263-370 (goal_mask "piid_allout", unseen.py:146-148): the piid arithmetic, but the result --
        always the MEAN of the action distribution at T-h, eval or not -- is left in ``self.action_list`` (one entry: the
        reference's further entries are commented out at 366-370) for the rollout loop to pop (learner.py:559-568).
        Returns None, as the reference does."""
        if eval:
            assert rtg is not None
        self.action_list = [self.action_piid_sample(sequence_history, percentage, horizon, plan, eval=True,
                                                    rtg=self._rtg_value(rtg, percentage))]
        return None

    @torch.no_grad()
    def goal_actions(self, states, actions, horizon: int, eval: bool = True, goal_mask: str = "piid", precision: Optional[str] = None,
                     want_window: bool = False):
        """The zero-shot action of E windows that are on the device already: states (E,T,S), actions (E,T,A) raw, one effective
        horizon for all of them (BASELINE config 5: thousands of goal-reaching windows per GPU).  Exactly pruned many-window path
        (m3pc_goal_step_batch): path inference reads the states head at the rows the overlay uses only, inverse dynamics reads
        ONE action token (zeroshot learner.py:240-256).  goal_mask "piid" (action_piid_sample) or "id" (action_id_sample).
        precision: "bf16" / "bf16x3" / "fp32"; default the planner's.  Returns (E, A): tanh(loc) when eval, a sample else."""
        prec = self.precision if precision is None else capi.precision_code(precision)
        idx = self.T - int(horizon)
        self._drain()  # (m3pc_goal_step_batch runs in the candidate workspace)
        res = self.handle.goal_step_batch(states, actions, idx, capi.GOAL_PIID if goal_mask == "piid" else capi.GOAL_ID, prec,
                                          want_window=want_window)
        mu, sd = res[0], res[1]
        if want_window:
            self.last = dict(window_states=res[2], loc=mu, std=sd)
        if eval:
            return torch.tanh(mu)
        # SquashedNormal.sample (mtm_model.py:263-269): the variates of the whole (E,T,1,A) distribution are drawn, as the
        # reference draws them, and the token's are used
        eps = self._eps((mu.shape[0], self.T, 1, self.A))[:, idx, 0]
        return torch.tanh(eps * sd + mu)

    @torch.no_grad()
    def action_piid_sample_batch(self, sequence_histories, percentage=1.0, eval=True, rtg=None, pruned: Optional[bool] = None,
                                 store=None, env_ids=None):
        """E independent goal-reaching windows per launch (BASELINE config 5 / SURVEY §8 f1): the reference plans one
        env per call (zeroshot learner.py:151-261, unseen.py rollout loop); here the windows that share a horizon go
        through the pi and fid forwards as ONE batch of the same kernels.  Per window the arithmetic is that of
        ``action_piid_sample``.  Returns (E, A).
        pruned=False (default up to 64 windows): the fp32 few-row kernels of ``action_piid_sample`` on the whole batch
        (``max_batch >= E``; ``last["state_inference"]`` holds every window's full states head).
        pruned=True (default beyond, needs ``goal_batch >= E``): the exactly pruned many-window path in the planner's
        precision (``goal_actions``).
        ``store``: an ``episodes.EpisodeStore`` holding the histories (way-points included) on the device: the windows of its
        environments ``env_ids`` (None: all) are assembled there (m3pc_episodes_windows, M3PC_WINDOW_GOAL) -- no per-window host
        loop and no H2D copy; ``sequence_histories`` is then ignored (pass None).  The windows are the bits of the host path's
        (for a store of 1000 steps, the reference's buffer length), so the results are too."""
        if eval:
            assert rtg is not None
        from .masks import create_fid_mask, create_pi_mask, mask_rows
        T = self.T
        S, A = self.S, self.A
        win = None if store is None else store.windows(env_ids, horizon=int(self.cfg.horizon), mode="goal")
        E = len(sequence_histories) if win is None else win[0].shape[0]
        if pruned is None:
            pruned = E > 64 or E > self._max_batch
        if pruned and E > self._goal_batch:
            raise ValueError(f"{E} windows through the pruned path need HipPlanner(..., goal_batch >= {E})"
                             + (f" (or, up to 64 windows, max_batch >= {E} for the un-pruned fp32 path: max_batch is {self._max_batch})"
                                if E <= 64 else ""))
        if win is None:
            host = np.empty((E, T * (S + A + 1)), dtype=np.float32)
            meta = [self._goal_window_host(hst, rtg, percentage, host[i]) for i, hst in enumerate(sequence_histories)]
            dev = torch.from_numpy(host).to(self.device)  # one packed H2D copy for all windows
        else:
            rtg_v = self._rtg_value(rtg, percentage)
            meta = [(int(h), rtg_v) for h in win[3]]
        out = torch.empty((E, self.A), dtype=torch.float32, device=self.device)
        infer = [None] * E
        self._drain()
        for h in sorted({m[0] for m in meta}):
            ids = [i for i, m in enumerate(meta) if m[0] == h]
            idx = T - h
            if win is None:
                sel = dev if len(ids) == E else dev[torch.tensor(ids, device=self.device)]
                s = sel[:, : T * S].reshape(-1, T, S).contiguous()
                a = sel[:, T * S : T * (S + A)].reshape(-1, T, A).contiguous()
            else:
                sel = None
                s, a, r = win[:3] if len(ids) == E else [x[torch.tensor(ids, device=self.device)] for x in win[:3]]
            if pruned:
                act = self.goal_actions(s, a, h, eval=eval)
                if len(ids) == E:
                    out = act
                else:
                    out[torch.tensor(ids, device=self.device)] = act
                continue
            if sel is not None:
                r = sel[:, T * (S + A) :].reshape(-1, T, 1).contiguous()
            mu, sd, inferred, _ = self.handle.goal_step(s, a, r, [meta[i][1] for i in ids], mask_rows(create_pi_mask(T, "cpu", idx)),
                                                        mask_rows(create_fid_mask(T, "cpu", idx)), idx)
            dist_ = SquashedNormal(mu.unsqueeze(2), sd.unsqueeze(2))
            act = dist_.mean if eval else dist_.sample(eps=self._eps(tuple(dist_.loc.shape)))
            out[torch.tensor(ids, device=self.device)] = act[:, idx, 0]
            for j, i in enumerate(ids):
                infer[i] = inferred[j]
        self._mark_main()
        # (the pruned path computes the states head on the rows the overlay reads only: there is no full per-window inference to
        # report -- said here instead of a list of None; goal_actions(want_window=True) gives the window rows)
        self.last = dict(state_inference=None if pruned else infer, pruned=bool(pruned))
        return out

    # ---------------------------------------------------------------------------------------- CEM refinement
    @torch.no_grad()
    def cem_guiding(self, trajectory: Dict[str, torch.Tensor], h: int, iterations: int = 2, top_k: int = 128, init_std: float = 0.1,
                    noise=None, native: bool = False, weighting: str = "cem", temperature: Optional[float] = None, min_std: float = 0.0,
                    init_mean=None):
        """Cross-entropy refinement of the plan (the legacy ``sample_action_cem`` of
        research/omtm/datasets/sequence_dataset.py:919-1000 -- N=1024, top_k=128, 2 iterations -- restated on this model's
        plan step: that function predates the four-key omtm model and cannot run on it, so parity is pinned on the oracle's
        restatement of the same algorithm (tests/test_batch_gpu.py), not on the reference).
          candidates_0 = clamp(tanh(policy loc) + init_std * noise_0, -1, 1) over the last h steps
          repeat: score (TD(lambda) as rtg_guiding / critic_lambda_guiding) -> top_k -> mean / std per (t, a)
                  candidates = clamp(mean + std * noise_i, -1, 1)
        Returns (sample_action (1,A): first action of candidate 0 after the last refit, as the legacy code returns;
                 eval_action (A,): first action of the final mean).  ``noise``: optional (iterations+1, N, h, A) normals.
        native=True: the whole refinement as ONE library call (m3pc_refine_plan: refit and resample on the device, nothing but
        the library's kernels), with what that call adds: weighting "cem" (equal weights on the top_k) or "mppi" (softmax of
        ``temperature`` x score over the top_k; default cfg.temperature), ``min_std`` (floor of every refit std) and ``init_mean``
        (h, A): the warm start, e.g. ``last["cem"][-1]["mean"]`` of the previous call, in place of tanh(policy loc).  Without
        ``noise`` it is drawn from torch as in the loop below, or by the library from (seed, step index) when the planner was
        built with variates="library".  native=False takes none of these options (ValueError)."""
        if native:
            return self._cem_native(trajectory, h, iterations, top_k, init_std, noise, weighting, temperature, min_std, init_mean)
        if weighting != "cem" or temperature is not None or min_std != 0.0 or init_mean is not None:
            raise ValueError("cem_guiding: weighting / temperature / min_std / init_mean need native=True")
        self._drain()
        s, a, r, rtg, ret = self._split(trajectory)
        cfg = self.cfg
        N, T, A = int(cfg.action_samples), self.T, self.A
        mode = capi.MODE_CRITIC if cfg.plan_guidance == "critic_lambda_guiding" else capi.MODE_RTG
        lmbda = 0.6 if mode == capi.MODE_RTG else float(cfg.lmbda)
        toks = [self.handle.tokenize(capi.STATES, s[None]), a[None], None, self._returns_tokens(rtg, ret)]
        from .masks import create_rcbc_mask, mask_rows
        mu, _ = self.handle.forward(toks, mask_rows(create_rcbc_mask(T, "cpu", T - h)), want=("actions",))["actions"]
        mean = torch.tanh(mu[0, T - h :])  # (h, A)
        std = torch.full_like(mean, float(init_std))
        if noise is None:
            noise = self._eps((iterations + 1, N, h, A))
        k = min(int(top_k), N)
        cand = torch.clamp(mean[None] + std[None] * noise[0], -1.0, 1.0)
        trace = []
        for it in range(iterations):
            er = self.handle.score_actions(mode, s, a, r, cand, None, h, lmbda, float(cfg.discount), precision=self.precision)
            top = torch.topk(er, k).indices
            elite = cand[top]
            mean = elite.mean(dim=0)
            std = elite.std(dim=0) if k > 1 else torch.zeros_like(mean)
            trace.append(dict(expect_return=er, top=top, mean=mean, std=std))
            cand = torch.clamp(mean[None] + std[None] * noise[it + 1], -1.0, 1.0)
        self._mark_main()
        self.last = dict(cem=trace, candidates=cand)
        return cand[0, 0][None], mean[0]

    def _cem_native(self, trajectory, h, iterations, top_k, init_std, noise, weighting, temperature, min_std, init_mean):
        """``cem_guiding(native=True)``: one m3pc_refine_plan call; fills ``self.last`` as the Python loop does."""
        if weighting not in capi.REFINE_WEIGHTINGS:
            raise ValueError(f"weighting must be one of {sorted(capi.REFINE_WEIGHTINGS)}, got {weighting!r}")
        self._drain()
        s, a, r, rtg, ret = self._split(trajectory)
        cfg = self.cfg
        N, A = int(cfg.action_samples), self.A
        mode = capi.MODE_CRITIC if cfg.plan_guidance == "critic_lambda_guiding" else capi.MODE_RTG
        lmbda = 0.6 if mode == capi.MODE_RTG else float(cfg.lmbda)
        k = min(int(top_k), N)
        seed = step = 0
        if noise is None:
            if self._variates == "library":
                seed, step, self._step_index = self._seed, self._step_index, self._step_index + 1
            else:
                noise = self._eps((iterations + 1, N, h, A))
        else:
            noise = noise.to(self.device, torch.float32).contiguous()
        tau = float(cfg.temperature) if temperature is None else float(temperature)
        res = self.handle.refine_plan(mode, s, a, r, h, rtg, lmbda, float(cfg.discount), N, iterations=iterations, top_k=k,
                                      weighting=capi.REFINE_WEIGHTINGS[weighting], temperature=tau, init_std=init_std, min_std=min_std,
                                      noise=noise, seed=seed, step=step, init_mean=init_mean, precision=self.precision, returns=ret)
        self._mark_main()
        trace = [dict(expect_return=res["scores"][it], top=res["elites"][it], mean=res["mean"][it + 1], std=res["std"][it + 1])
                 for it in range(iterations)]
        self.last = dict(cem=trace, candidates=res["candidates"])
        return res["sample_action"], res["eval_action"]

    @torch.no_grad()
    def cem_guiding_batch(self, trajectories, h: int, iterations: int = 2, top_k: int = 128, init_std: float = 0.1, noise=None,
                          weighting: str = "cem", temperature: Optional[float] = None, min_std: float = 0.0, init_mean=None,
                          init_rows=None, init_offset: int = 0):
        """``cem_guiding(native=True)`` for E windows that step together, as ONE library call (m3pc_refine_plans: one policy pass
        at batch E, per iteration one scoring pass over the E x N candidates, one top-k, one refit, one resample).  trajectories:
        E reference-style dicts of (1,T,D) tensors with a constant return-to-go (``_rtg``), all of effective horizon ``h``; needs
        ``HipPlanner(..., max_batch=E, max_windows=E)``.  noise: optional (iterations+1, E, N, h, A) normals; without it torch
        draws them, or the library does from (seed, step index + w) when the planner was built with variates="library" (the index
        advances by E).  init_mean (E, rows, A), init_rows (E,), init_offset: the shifted warm start -- row t of window w starts
        from init_mean[w, t + init_offset] while t + init_offset < init_rows[w] (default: every row given), else from tanh of the
        policy loc; ``init_rows[w] = 0``: a cold start.
        Returns (sample_action (E,A), eval_action (E,A)); ``self.last["cem"][w]`` is the trace ``cem_guiding`` fills, per window."""
        trajectories = list(trajectories)
        parts = [self._split(t) for t in trajectories]
        if any(ret is not None for *_, ret in parts):
            raise ValueError("cem_guiding_batch takes a constant return-to-go per window (trajectory['_rtg']), not a returns row")
        s, a, r = (torch.stack([q[i] for q in parts]).contiguous() for i in range(3))
        return self._cem_batch(s, a, r.reshape(len(parts), self.T, 1), [q[3] for q in parts], h, iterations, top_k, init_std, noise,
                               weighting, temperature, min_std, init_mean, init_rows, init_offset)

    def _cem_batch(self, s, a, r, rtgs, h, iterations, top_k, init_std, noise, weighting, temperature, min_std, init_mean, init_rows,
                   init_offset):
        """``cem_guiding_batch`` on stacked windows s (E,T,S), a (E,T,A), r (E,T,1) and their return-to-go values."""
        if weighting not in capi.REFINE_WEIGHTINGS:
            raise ValueError(f"weighting must be one of {sorted(capi.REFINE_WEIGHTINGS)}, got {weighting!r}")
        cfg = self.cfg
        if cfg.plan_guidance == "noise_adding_lambda":
            raise ValueError("refinement scores with rtg_guiding or critic_lambda_guiding; noise_adding_lambda has no scoring of its own")
        self._drain()
        E, N, A = int(s.shape[0]), int(cfg.action_samples), self.A
        mode = capi.MODE_CRITIC if cfg.plan_guidance == "critic_lambda_guiding" else capi.MODE_RTG
        lmbda = 0.6 if mode == capi.MODE_RTG else float(cfg.lmbda)
        k = min(int(top_k), N)
        seed, steps = 0, None
        if noise is None:
            if self._variates == "library":
                seed, steps = self._seed, [self._step_index + w for w in range(E)]
                self._step_index += E
            else:
                noise = self._eps((iterations + 1, E, N, h, A))
        else:
            noise = noise.to(self.device, torch.float32).contiguous()
        tau = float(cfg.temperature) if temperature is None else float(temperature)
        res = self.handle.refine_plans(mode, s, a, r, h, rtgs, lmbda, float(cfg.discount), N, iterations=iterations, top_k=k,
                                       weighting=capi.REFINE_WEIGHTINGS[weighting], temperature=tau, init_std=init_std, min_std=min_std,
                                       noise=noise, seed=seed, steps=steps, init_mean=init_mean, init_rows=init_rows,
                                       init_offset=init_offset, precision=self.precision)
        self._mark_main()
        trace = [[dict(expect_return=res["scores"][it, w], top=res["elites"][it, w], mean=res["mean"][it + 1, w], std=res["std"][it + 1, w])
                  for it in range(iterations)] for w in range(E)]
        self.last = dict(cem=trace, candidates=res["candidates"], mean=res["mean"], std=res["std"])
        return res["sample_action"], res["eval_action"]
