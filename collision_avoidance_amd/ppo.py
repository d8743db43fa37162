"""A small PPO trainer on top of rollout_policy_sample(): the reference's shared-weights 64-64 ReLU model with a value head on its
last hidden layer and a state-independent log-std (reference run_rllib.py:35-52, 96-125: gamma 0.95, 10 SGD passes per batch).

The batch comes from the device in one call -- observations, eps, log-probabilities, the distribution's parameters, values,
advantages and value targets; torch is used for the gradient steps alone.  After an update the weights are installed
again with set_policy() / set_policy_heads(), so the next collect() samples from the policy that was just trained.

The log-probability the library records is defined as a k-ordered fmaf chain; torch's GEMM adds in another order, so the importance
ratio of the first minibatch is 1 to rounding, not exactly.

With env.set_reward_terms(...) the rewards, advantages and value targets of the batch are those of the shaped reward -- collision,
wall, arrival and time terms computed on the device between the steps --, and nothing here changes."""
import math

import numpy as np
import torch


class PPOTrainer:
    def __init__(self, env, hidden=(64, 64), gamma=0.95, lam=0.95, clip=0.2, lr=3e-4, sgd_iters=10, minibatch=4096, vf_coef=0.5,
                 log_std_init=-0.5, out="clip", limit=math.pi, hold=1):
        if not env.use_torch:
            raise ValueError("PPOTrainer: the environment must be made with use_torch=True")
        self.env, self.gamma, self.lam, self.clip, self.sgd_iters, self.minibatch = env, float(gamma), float(lam), float(clip), int(sgd_iters), int(minibatch)
        self.vf_coef, self.out, self.limit, self.hold = float(vf_coef), out, float(limit), int(hold)
        dev = torch.device("cuda", env.device)
        mods, w = [], 64
        for h in hidden:
            mods += [torch.nn.Linear(w, int(h)), torch.nn.ReLU()]
            w = int(h)
        self.trunk = torch.nn.Sequential(*mods).to(dev)
        self.mean_head = torch.nn.Linear(w, 1).to(dev)
        self.value_head = torch.nn.Linear(w, 1).to(dev)
        self.log_std = torch.nn.Parameter(torch.full((1,), float(log_std_init), device=dev))
        self.opt = torch.optim.Adam(self.parameters(), lr=lr)
        self.install()

    def parameters(self):
        return list(self.trunk.parameters()) + list(self.mean_head.parameters()) + list(self.value_head.parameters()) + [self.log_std]

    def layers(self):
        """([(W, b)] of the policy, (value_w [1, K], value_b [1]), (None, log_std_b [1])) as host arrays: what install() installs"""
        host = lambda t: t.detach().cpu().numpy().astype(np.float32)
        lin = [m for m in self.trunk if isinstance(m, torch.nn.Linear)] + [self.mean_head]
        return [(host(m.weight), host(m.bias)) for m in lin], (host(self.value_head.weight), host(self.value_head.bias)), (None, host(self.log_std))

    def install(self):
        layers, value, log_std = self.layers()
        self.env.set_policy(layers, out=self.out, limit=self.limit)
        self.env.set_policy_heads(value=value, log_std=log_std)

    def collect(self, steps):
        """One batch of `steps` steps from the state the environment is in: the records of rollout_policy_sample() and the eps drawn"""
        R = (int(steps) + self.hold - 1) // self.hold
        eps = torch.randn((R, self.env.A, self.env.N), dtype=torch.float32, device=torch.device("cuda", self.env.device))
        batch = self.env.rollout_policy_sample(steps, hold=self.hold, noise=eps, gamma=self.gamma, lam=self.lam, autoreset=True)
        batch["eps"] = eps
        return batch

    def update(self, batch):
        """Clipped-surrogate PPO and a value loss on the device records; then install().  Returns the last minibatch's losses and the
        first minibatch's importance ratio (mean and largest deviation from 1)."""
        obs = batch["obs"].reshape(-1, 64)
        mean0, ls0 = batch["dist"][:, 0].reshape(-1), batch["dist"][:, 1].reshape(-1)
        # the unclipped sample u = mean + std * eps, rebuilt from the recorded distribution: under out="clip" the action is not u
        u = mean0 + torch.exp(ls0) * batch["eps"].reshape(-1)
        logp0, adv, tgt = batch["logp"].reshape(-1), batch["advantages"].reshape(-1), batch["targets"].reshape(-1)
        keep = batch["row_valid"].bool()[:, :, None].expand(-1, -1, self.env.N).reshape(-1)
        idx = torch.nonzero(keep).reshape(-1)
        adv = (adv - adv[idx].mean()) / (adv[idx].std() + 1e-8)
        info = {}
        for it in range(self.sgd_iters):
            perm = idx[torch.randperm(idx.numel(), device=idx.device)]
            for k in range(0, perm.numel(), self.minibatch):
                mb = perm[k:k + self.minibatch]
                h = self.trunk(obs[mb])
                mean, value = self.mean_head(h).reshape(-1), self.value_head(h).reshape(-1)
                ls = self.log_std.clamp(-20.0, 2.0)
                z = (u[mb] - mean) * torch.exp(-ls)
                logp = -0.5 * z * z - ls - 0.918938533
                ratio = torch.exp(logp - logp0[mb])
                if not info:
                    info["ratio_first_mean"] = ratio.detach().mean().item()
                    info["ratio_first_dev"] = (ratio.detach() - 1).abs().max().item()
                pi_loss = -torch.min(ratio * adv[mb], ratio.clamp(1 - self.clip, 1 + self.clip) * adv[mb]).mean()
                v_loss = (value - tgt[mb]).pow(2).mean()
                loss = pi_loss + self.vf_coef * v_loss
                self.opt.zero_grad()
                loss.backward()
                self.opt.step()
        info.update(pi_loss=pi_loss.item(), v_loss=v_loss.item(), loss=loss.item())
        self.install()
        return info
