"""PPO + LSTM rate-controller policy in PyTorch-ROCm.

Architecture = what the reference's `train_rate.py:115-147` builds: sb3_contrib `RecurrentPPO("MlpLstmPolicy")` with
`LSTMPolicy.get_policy_kwargs()` (learned_controllers/networks/lstm_policy.py:107-136):

  features extractor (lstm_policy.py:13-97): Linear(18,128)+ReLU -> nn.LSTM(128,256,num_layers=2) -> Linear(256,128)+ReLU
      NOTE the reference calls `self.lstm(embedded)` on a length-1 sequence WITHOUT carried state (:75-92), so this
      2-layer LSTM always starts from h=c=0: the W_hh products and the forget gate vanish and each layer reduces to
      h = sigmoid(o) * tanh(sigmoid(i) * tanh(g)) with gates = x W_ih^T + b_ih + b_hh.  We keep nn.LSTM's parameter
      tensors (checkpoint-compatible) but evaluate that closed form: one GEMM per layer instead of two.
  actor LSTM / critic LSTM (sb3_contrib defaults): nn.LSTM(128, 256, 1) each, state carried across env steps and
      zeroed at episode starts -- THE recurrence, and the only dense contraction with a sequential dependency;
  mlp_extractor: pi [128, 64], vf [128, 64], ReLU;  action_net Linear(64,4), value_net Linear(64,1), log_std (4).
SB3 / sb3_contrib are third-party and absent here: numerics parity with them is unpinned; shapes,
parameter names and hyper-parameters follow the reference's config (learned_controllers/config/ppo_lstm.yaml:38-58).

Every matmul is a `[B, K] x [K, 4H]` GEMM that rocBLAS/hipBLASLt runs on MFMA; with `compute_dtype=torch.bfloat16`
the GEMMs run in bf16 with fp32 accumulate (autocast), the cell state and the PPO loss stay fp32.
"""
import math
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import inference
from .fused import DeferredWgrad, deferred_linear, linear, linear_relu, lstm_cell, lstm_sequence, zero_state_lstm_layer
from .inference import FE_GATE_SCALE, _KPERM16, _kperm, pack_fe_weights      # noqa: F401  (the weight packers moved with the snapshot)

OBS_DIM, ACT_DIM = 18, 4


class RNNStates(NamedTuple):
    pi_h: torch.Tensor   # [B, H]
    pi_c: torch.Tensor
    vf_h: torch.Tensor
    vf_c: torch.Tensor

    def detach(self):
        return RNNStates(*(t.detach() for t in self))

    def masked(self, keep):
        """keep = 1 - episode_start, [B] -> zero the state of envs that start a new episode."""
        k = keep.unsqueeze(-1)
        return RNNStates(*(t * k.to(t.dtype) for t in self))

    def index(self, idx):
        return RNNStates(*(t[idx] for t in self))


def _lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """One LSTM step: ONE GEMM over the concatenated [x, h] (K = in + H, MFMA via hipBLASLt; PyTorch gate order
    i, f, g, o) followed by ONE fused point-wise launch (fused.lstm_cell)."""
    gates = F.linear(torch.cat([x, h.to(x.dtype)], dim=-1), torch.cat([w_ih, w_hh], dim=1), b_ih + b_hh)
    return lstm_cell(gates, c)


def _lstm_zero_state_layer(x, w_ih, b_ih, b_hh):
    return zero_state_lstm_layer(x, w_ih, b_ih, b_hh)


def _run_seq(seq, x):
    """nn.Sequential of Linear / ReLU, with the Linears routed through fused.linear (split-K weight gradients) and a
    Linear + ReLU pair through fused.linear_relu (bias + ReLU in the GEMM epilogue)."""
    mods, i = list(seq), 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Linear) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU) and m.bias is not None:
            x = linear_relu(x, m.weight, m.bias)
            i += 2
            continue
        x = linear(x, m.weight, m.bias) if isinstance(m, nn.Linear) else m(x)
        i += 1
    return x


class LSTMFeaturesExtractor(nn.Module):
    def __init__(self, obs_dim: int = OBS_DIM, features_dim: int = 128, lstm_hidden_size: int = 256, n_lstm_layers: int = 2):
        super().__init__()
        self.features_dim = features_dim
        self.embedding = nn.Sequential(nn.Linear(obs_dim, 128), nn.ReLU())
        self.lstm = nn.LSTM(input_size=128, hidden_size=lstm_hidden_size, num_layers=n_lstm_layers, batch_first=True)
        self.output_proj = nn.Sequential(nn.Linear(lstm_hidden_size, features_dim), nn.ReLU())

    def forward(self, obs):
        x = _run_seq(self.embedding, obs)
        for layer in range(self.lstm.num_layers):
            x = _lstm_zero_state_layer(x, getattr(self.lstm, f"weight_ih_l{layer}"), getattr(self.lstm, f"bias_ih_l{layer}"),
                                       getattr(self.lstm, f"bias_hh_l{layer}")).to(x.dtype)
        return _run_seq(self.output_proj, x)


def _mlp(sizes):
    layers = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        layers += [nn.Linear(a, b), nn.ReLU()]
    return nn.Sequential(*layers)


class RateLSTMPolicy(nn.Module):
    """Actor-critic with separate actor/critic LSTMs (sb3_contrib RecurrentActorCriticPolicy defaults)."""

    def __init__(self, features_dim: int = 128, lstm_hidden_size: int = 256, n_lstm_layers: int = 2,
                 policy_lstm_hidden: int = 256, net_arch_pi=(128, 64), net_arch_vf=(128, 64), use_lstm: bool = True,
                 mlp_net_arch=(256, 128, 64), compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.use_lstm, self.hidden, self.compute_dtype = use_lstm, policy_lstm_hidden, compute_dtype
        self.deferred_wgrad = True       # BPTT: one split-K weight-gradient GEMM per recurrent cell per backward pass
        self.sequence_bptt = True        # BPTT: each recurrent cell over T steps is one autograd node (fused.lstm_sequence)
        self.group_cells_max_batch = 8192    # slices up to this many envs run actor + critic cells as one batched node
        if use_lstm:
            self.features_extractor = LSTMFeaturesExtractor(OBS_DIM, features_dim, lstm_hidden_size, n_lstm_layers)
            self.lstm_actor = nn.LSTM(features_dim, policy_lstm_hidden, 1)
            self.lstm_critic = nn.LSTM(features_dim, policy_lstm_hidden, 1)
            self.pi_net = _mlp([policy_lstm_hidden, *net_arch_pi])
            self.vf_net = _mlp([policy_lstm_hidden, *net_arch_vf])
            last_pi, last_vf = net_arch_pi[-1], net_arch_vf[-1]
        else:   # SimpleMLPPolicy (lstm_policy.py:139-164): PPO("MlpPolicy"), pi = vf = mlp.net_arch
            self.features_extractor = nn.Identity()
            self.pi_net = _mlp([OBS_DIM, *mlp_net_arch])
            self.vf_net = _mlp([OBS_DIM, *mlp_net_arch])
            last_pi = last_vf = mlp_net_arch[-1]
        self.action_net = nn.Linear(last_pi, ACT_DIM)
        self.value_net = nn.Linear(last_vf, 1)
        self.log_std = nn.Parameter(torch.zeros(ACT_DIM))
        self._init_weights()

    def _init_weights(self):
        # SB3 ortho_init: sqrt(2) for the trunks, 0.01 for the action head, 1 for the value head
        for mod, gain in ((self.features_extractor, math.sqrt(2)), (self.pi_net, math.sqrt(2)), (self.vf_net, math.sqrt(2)),
                          (self.action_net, 0.01), (self.value_net, 1.0)):
            for m in mod.modules():
                if isinstance(m, nn.Linear):
                    nn.init.orthogonal_(m.weight, gain=gain)
                    nn.init.zeros_(m.bias)

    def initial_state(self, batch: int, device=None) -> RNNStates:
        z = lambda: torch.zeros(batch, self.hidden, device=device or self.log_std.device)  # noqa: E731
        return RNNStates(z(), z(), z(), z())

    # ---- single env step (rollout) --------------------------------------------------------------------------
    def _core(self, obs, states: RNNStates):
        feats = self.features_extractor(obs)
        if not self.use_lstm:
            return self.pi_net(feats), self.vf_net(feats), states
        la, lc = self.lstm_actor, self.lstm_critic
        pi_h, pi_c = _lstm_cell(feats, states.pi_h, states.pi_c, la.weight_ih_l0, la.weight_hh_l0, la.bias_ih_l0, la.bias_hh_l0)
        vf_h, vf_c = _lstm_cell(feats, states.vf_h, states.vf_c, lc.weight_ih_l0, lc.weight_hh_l0, lc.bias_ih_l0, lc.bias_hh_l0)
        return self.pi_net(pi_h), self.vf_net(vf_h), RNNStates(pi_h, pi_c, vf_h, vf_c)

    # ---- fused inference path (inference.py): every LSTM cell is ONE hand-written MFMA kernel (csrc/lstm_mfma.hip) ----------
    _inf: Optional[inference.Snapshot] = None      # plain attribute: not a module, buffer or parameter, absent from state_dict()

    def prepare_inference(self):
        """Snapshot the weights for the fused rollout path (None where its kernels do not serve this policy's shapes: the plain
        path runs then).  Call after every optimizer phase (RecurrentPPO.collect_rollout does); the snapshot is refreshed IN
        PLACE and the training path never reads it."""
        self._inf = inference.prepare(self._inf, self)

    def _fused_ok(self, obs):
        return (self._inf is not None and obs.is_cuda and self.compute_dtype == torch.bfloat16 and not torch.is_grad_enabled()
                and not inference.knob("FDYN_NO_MFMA"))

    def recurrent_inplace_ok(self, batch: int, device) -> bool:
        """True if the fused rollout path may update the recurrent state of `batch` envs IN PLACE (one state set instead of a
        ping-pong pair: the footprint that decides whether the state survives in the Infinity Cache between steps)."""
        return (self.compute_dtype == torch.bfloat16 and torch.device(device).type == "cuda" and inference.served(self)
                and inference.inplace_ok(batch))

    def noise_counter(self, device):
        """The device-side step counter of the fused path's action noise (created on first use)."""
        if not hasattr(self, "_noise_seed"):
            self._noise_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            self._noise_step = torch.zeros(1, dtype=torch.int32, device=device)
        return self._noise_step

    def step(self, obs, states: RNNStates, episode_start, deterministic: bool = False,
             out_states: Optional[RNNStates] = None, keep: Optional[torch.Tensor] = None, bump_noise: bool = True,
             done_flags: Optional[tuple] = None):
        """obs [B,18], episode_start [B] (1 where the env was just reset) -> actions, values, log_probs, new states.
        keep: 1 - episode_start if the caller already has it (fused.episode_flags writes both); bump_noise=False: the caller
        moves the noise counter on itself (the same launch) -- a rollout loop then has no framework glue launches left.
        done_flags = (terminated, truncated) of the PREVIOUS env step (fused path only, with `keep` given): episode_start and keep
        are REWRITTEN from them and the noise counter moves on inside the step's first kernel."""
        if self._fused_ok(obs):
            counter = self.noise_counter(obs.device)
            *out, new_states = inference.step(self._inf, (self.log_std, self._noise_seed, counter), obs, states, episode_start,
                                              deterministic, out_states, keep, bump_noise, done_flags)
            return (*out, RNNStates(*new_states))
        states = states.masked(1.0 - episode_start.float())
        with torch.autocast(obs.device.type, dtype=self.compute_dtype, enabled=self.compute_dtype is not None):
            lat_pi, lat_vf, new_states = self._core(obs, states)
            mean = self.action_net(lat_pi).float()
            value = self.value_net(lat_vf).float().squeeze(-1)
        std = self.log_std.exp()
        actions = mean if deterministic else mean + std * torch.randn_like(mean)
        return actions, value, self._log_prob(actions, mean), new_states

    def _log_prob(self, actions, mean):
        var = (2 * self.log_std).exp()
        return (-((actions - mean) ** 2) / (2 * var) - self.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)

    def entropy(self):
        return (0.5 + 0.5 * math.log(2 * math.pi) + self.log_std).sum()

    # ---- sequence evaluation (PPO update, BPTT over T) ----------------------------------------------------------
    def evaluate_sequence(self, obs, actions, episode_starts, states: RNNStates) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """obs [T,B,18], actions [T,B,4], episode_starts [T,B], states at t=0 -> values [T,B], log_probs [T,B], entropy."""
        values, mean = self.sequence_heads(obs, episode_starts, states)
        return values, self._log_prob(actions, mean), self.entropy()

    def sequence_heads(self, obs, episode_starts, states: RNNStates) -> Tuple[torch.Tensor, torch.Tensor]:
        """BPTT forward over T steps: obs [T,B,18], episode_starts [T,B], states at t=0 -> values [T,B], action means [T,B,4]."""
        T = obs.shape[0]
        with torch.autocast(obs.device.type, dtype=self.compute_dtype, enabled=self.compute_dtype is not None):
            if not self.use_lstm:
                flat = obs.reshape(-1, OBS_DIM)
                lat_pi, lat_vf = _run_seq(self.pi_net, flat), _run_seq(self.vf_net, flat)
                mean = linear(lat_pi, self.action_net.weight, self.action_net.bias).float().view(T, -1, ACT_DIM)
                values = linear(lat_vf, self.value_net.weight, self.value_net.bias).float().view(T, -1)
                return values, mean
            # the zero-state feature extractor has no time dependence: run it for all T*B rows in one set of GEMMs
            feats = self.features_extractor(obs.reshape(-1, OBS_DIM)).view(T, -1, self.features_extractor.features_dim)
            la, lc = self.lstm_actor, self.lstm_critic
            wa, ba = torch.cat([la.weight_ih_l0, la.weight_hh_l0], 1), la.bias_ih_l0 + la.bias_hh_l0
            wc, bc = torch.cat([lc.weight_ih_l0, lc.weight_hh_l0], 1), lc.bias_ih_l0 + lc.bias_hh_l0
            pi_h, pi_c, vf_h, vf_c = states
            if self.sequence_bptt and feats.is_cuda:
                # the actor and critic cells over all T steps are ONE autograd node (fused.lstm_sequence): per step and
                # direction one batched GEMM + one point-wise launch for both cells, weight gradients from one batched GEMM
                keep_all = 1.0 - episode_starts.float()
                cells = [(l.weight_ih_l0, l.weight_hh_l0, l.bias_ih_l0, l.bias_hh_l0) for l in (la, lc)]
                dt = feats.dtype
                if feats.shape[1] <= self.group_cells_max_batch:
                    # small slices: both cells in one node (halves the launches; measured 244 -> 214 ms at 2048-env slices)
                    h_seq, _ = lstm_sequence(feats, cells, torch.stack([pi_h.to(dt), vf_h.to(dt)]), torch.stack([pi_c, vf_c]), keep_all)
                    pi_seq, vf_seq = h_seq.unbind(1)       # backward = one stack copy (two selects: two zero fills + an add)
                else:
                    # large slices fill the chip per cell; the batched GEMM is then slower than two plain ones (74 vs 68 ms)
                    pi_seq = lstm_sequence(feats, cells[:1], pi_h.to(dt).unsqueeze(0), pi_c.unsqueeze(0), keep_all)[0].squeeze(1)
                    vf_seq = lstm_sequence(feats, cells[1:], vf_h.to(dt).unsqueeze(0), vf_c.unsqueeze(0), keep_all)[0].squeeze(1)
                mean = linear(_run_seq(self.pi_net, pi_seq), self.action_net.weight, self.action_net.bias).float()
                values = linear(_run_seq(self.vf_net, vf_seq), self.value_net.weight, self.value_net.bias).float().squeeze(-1)
                return values, mean
            pi_hs, vf_hs = [], []
            # per-step autograd with deferred weight gradients (fused.DeferredWgrad): each step's backward only produces dX;
            # dW / db of the two recurrent cells come from one split-K GEMM over all T*B rows when the backward pass ends
            defer = self.deferred_wgrad and feats.is_cuda and torch.is_grad_enabled()
            if defer:
                Bn, kx, dt = feats.shape[1], feats.shape[2], feats.dtype
                wa, ba, wc, bc = wa.detach().to(dt), ba.detach().to(dt), wc.detach().to(dt), bc.detach().to(dt)
                mk = lambda l, w: DeferredWgrad(T, Bn, w.shape[1], w.shape[0], dt, feats.device,   # noqa: E731
                                                [(l.weight_ih_l0, slice(0, kx)), (l.weight_hh_l0, slice(kx, w.shape[1]))],
                                                [l.bias_ih_l0, l.bias_hh_l0])
                bk_a, bk_c = mk(la, wa), mk(lc, wc)
            for t in range(T):
                keep = (1.0 - episode_starts[t].float()).unsqueeze(-1)
                kh = keep.to(pi_h.dtype)
                pi_h, pi_c, vf_h, vf_c = pi_h * kh, pi_c * keep, vf_h * kh, vf_c * keep
                x = feats[t]
                if defer:
                    pi_h, pi_c = lstm_cell(deferred_linear(x, pi_h.to(x.dtype), wa, ba, bk_a, t), pi_c)
                    vf_h, vf_c = lstm_cell(deferred_linear(x, vf_h.to(x.dtype), wc, bc, bk_c, t), vf_c)
                else:
                    pi_h, pi_c = lstm_cell(F.linear(torch.cat([x, pi_h.to(x.dtype)], -1), wa, ba), pi_c)
                    vf_h, vf_c = lstm_cell(F.linear(torch.cat([x, vf_h.to(x.dtype)], -1), wc, bc), vf_c)
                pi_hs.append(pi_h); vf_hs.append(vf_h)
            pi_seq, vf_seq = torch.stack(pi_hs), torch.stack(vf_hs)
            mean = linear(_run_seq(self.pi_net, pi_seq), self.action_net.weight, self.action_net.bias).float()
            values = linear(_run_seq(self.vf_net, vf_seq), self.value_net.weight, self.value_net.bias).float().squeeze(-1)
        return values, mean

    def predict_values(self, obs, states: RNNStates, episode_start):
        return self.step(obs, states, episode_start, deterministic=True)[1]

    def num_parameters(self):
        return sum(p.numel() for p in self.parameters())

    @staticmethod
    def flops_per_env_step(use_lstm: bool = True) -> float:
        """Forward multiply-add flops per env step (2*K*N per row): embedding + 2 zero-state layers + proj + 2 LSTMs + heads."""
        if not use_lstm:
            return 2.0 * 2 * (18 * 256 + 256 * 128 + 128 * 64) + 2 * (64 * 4 + 64)
        return 2.0 * (18 * 128 + 128 * 1024 + 256 * 1024 + 256 * 128 + 2 * (384 * 1024) + 2 * (256 * 128 + 128 * 64) + 64 * 4 + 64)
