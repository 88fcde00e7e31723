"""Learned hand belief: a policy-aware head over the exact belief, trained from recorded games on the device.

Every search here samples the searcher's hidden hand from the PUBLIC belief (env.determinize / determinize_exact): uniform over the
unseen physical cards the card knowledge allows.  What the partner's moves say under the conventions of the policy being played is
not in it.  BeliefHead puts a linear head on the blueprint's frozen trunk (the top LSTM output at the step, computed from the seat's
own observation sequence from zero state, as cloning does) whose logits tilt the exact belief slot by slot:

    p_i[t] = w_i[t] exp(z[i 25 + t]) / sum_t' w_i[t'] exp(z[i 25 + t']),   w_i[t] = q[t] compat_i[t] C(slots after i, q - e_t)

(include/hsad.h, hsad_belief_tail; the row is csrc/hsad_belief_head.h).  With zero weights -- how a head is created -- the model IS
determinize_exact's distribution; every sampled hand is consistent with the card knowledge and the card counts whatever the logits;
and because the trunk is frozen and the head linear, the negative log-likelihood is convex in the head's parameters.

  BeliefHead.features / logits / loss / step / sample / save / load
  sequences_from_records(..., knowledge=True) (clone.py) carries env.hand_knowledge() of every kept step as the labels

    python -m hanabi_sad_amd.belief --blueprint FILE.pthw (--teacher NAME|FILE ... | --games FILE [--seat ..]) --num_game N --sad 1 \\
           --num_epoch E --batchsize B --holdout 0.1 --lr 1e-3 --save_dir D

In the searches: BeliefSampler holds a head's two tensors and turns the acting agent's state after the root act into logits
(hsad_search_belief_rows, then the head's GEMM); search.PolicySearch(sampler="learned", belief=...) draws every world's hand with
env.determinize_belief_worlds under them, the worlds of a game stratified slot by slot (csrc/hsad_belief_world.h).

Not here: training the trunk through the head, a hidden layer, a temperature, seats other than the viewer's own hand."""
import os

import numpy as np
import torch

from . import _lib
from . import game_record as gr

TYPES = 25


def _s(dev):
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def check_head_args(hand_size, H):
    """ValueError unless a head of this shape can exist: hands of 1..5 slots (the exact counting arithmetic's limit), a trunk width
    that is a positive multiple of 64 (the bf16 GEMM's k tile)"""
    if not 1 <= int(hand_size) <= 5:
        raise ValueError("hand_size %s: the belief counts hands of 1..5 slots" % hand_size)
    if int(H) < 64 or int(H) % 64:
        raise ValueError("trunk width %s: the head's GEMMs need a positive multiple of 64" % H)
    return int(hand_size), int(H)


def padded_logits(hand_size):
    """columns of the logits / gradient buffers: 25 per slot, rounded up to a multiple of 8 (bf16 rows of 16 bytes)"""
    return (TYPES * int(hand_size) + 7) // 8 * 8


def check_batch(batch, hand_size):
    """the shapes BeliefHead.loss needs of a batch -> (T, B); ValueError otherwise"""
    for k in ("o16", "pool", "compat", "cards", "seq_len"):
        if k not in batch:
            raise ValueError("the batch has no %r (make the dataset with sequences_from_records(..., knowledge=True) and "
                             "BeliefHead.features)" % k)
    o16, pool, compat, cards, seq_len = (batch[k] for k in ("o16", "pool", "compat", "cards", "seq_len"))
    if o16.dim() != 3 or o16.dtype != torch.bfloat16:
        raise ValueError("o16 must be bfloat16 [T, B, H]; got %s %s" % (o16.dtype, tuple(o16.shape)))
    T, B = int(o16.shape[0]), int(o16.shape[1])
    want = {"pool": ((T, B), torch.int64), "compat": ((T, B, hand_size), torch.int32), "cards": ((T, B, hand_size), torch.int32),
            "seq_len": ((B,), torch.float32)}
    for k, (shape, dtype) in want.items():
        if tuple(batch[k].shape) != shape or batch[k].dtype != dtype:
            raise ValueError("%s must be %s %s; got %s %s" % (k, dtype, shape, batch[k].dtype, tuple(batch[k].shape)))
    return T, B


class BeliefStats(dict):
    """nll, nll0 float32 [B] (sums over the sequence), cards, hits, hits0, bad int32 [B]; per_card() -> host floats"""

    def per_card(self):
        n = max(int(self["cards"].sum()), 1)
        return dict(nll=float(self["nll"].double().sum()) / n, nll0=float(self["nll0"].double().sum()) / n, top1=int(self["hits"].sum()) / n,
                    top1_0=int(self["hits0"].sum()) / n, cards=n, bad=int(self["bad"].sum()))


class BeliefHead:
    """the head: fp32 masters belief.weight [hand_size * 25, H] and belief.bias, zero at creation (= the exact public belief), their
    bf16 operand, Adam state; the blueprint's trunk, frozen.  blueprint: a weight dict or the path of a .pthw file."""

    def __init__(self, blueprint, hand_size=5, device="cuda:0", lr=1e-3, eps=1e-8, grad_clip=None):
        from .checkpoint import load_weights
        from .r2d2 import R2D2NetKernels, arch_of
        W = load_weights(blueprint) if isinstance(blueprint, (str, os.PathLike)) else blueprint
        hand_size, H = check_head_args(hand_size, W["fc_a.weight"].shape[1])
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HsadError("BeliefHead needs a ROCm device (got %s); there is no CPU path" % device)
        if tuple(arch_of(W)) != (1, 2):
            raise _lib.HsadError("BeliefHead runs the blueprint's trunk on the default architecture (1 fc layer, 2 LSTM layers); the composite "
                                 "entry points have no trunk-output call yet")
        self.lib = _lib.load_library()
        self.net = R2D2NetKernels(W, self.device)
        self.hand_size, self.H, self.NZ, self.NZp = hand_size, H, TYPES * hand_size, padded_logits(hand_size)
        d = self.device
        n_w = self.NZp * H
        self.flat = torch.zeros(n_w + self.NZp, dtype=torch.float32, device=d)       # [weight rows (padded) | bias (padded)]
        self.gflat, self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.w32, self.b32 = self.flat[:n_w].view(self.NZp, H), self.flat[n_w:]
        self.gw, self.gb = self.gflat[:n_w].view(self.NZp, H), self.gflat[n_w:]
        self.w16 = torch.zeros(self.NZp, H, dtype=torch.bfloat16, device=d)
        self.scratch = torch.zeros(4, dtype=torch.float32, device=d)
        self.lr, self.eps, self.grad_clip, self.step_count = float(lr), float(eps), grad_clip, 0
        self.wgrad_split = 8
        self._buf = {}

    # -- parameters --
    @property
    def weight(self):
        return self.w32[:self.NZ]

    @property
    def bias(self):
        return self.b32[:self.NZ]

    def refresh(self):
        """the bf16 operand from the fp32 master"""
        _lib.check(self.lib.hsad_prepare_weight(self.w32.data_ptr(), self.NZp, self.H, self.w32.stride(0), None, self.w16.data_ptr(),
                                                self.w16.stride(0), None, 0, _s(self.device)))

    def state(self):
        return {"belief.weight": self.weight.detach().cpu().clone(), "belief.bias": self.bias.detach().cpu().clone(),
                "hand_size": self.hand_size, "H": self.H}

    def save(self, path):
        torch.save(self.state(), path)

    def load(self, path_or_state):
        sd = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, (str, os.PathLike)) else path_or_state
        check_state(sd, self.hand_size, self.H)
        self.flat.zero_()
        self.weight.copy_(sd["belief.weight"].to(self.device, torch.float32))
        self.bias.copy_(sd["belief.bias"].to(self.device, torch.float32))
        self.refresh()
        return self

    # -- forward --
    def features(self, priv_s, rows_per_pass=512):
        """priv_s float32 [T, N, F] or bfloat16 [T, N, in_dim_padded] (CloneDataset.priv_s / .priv_s_bf16) -> the blueprint's top LSTM
        output bf16 [T, N, H], every sequence from zero state"""
        from .r2d2 import gemm_nt, lstm_layer_forward
        net, H = self.net, self.H
        T, N = int(priv_s.shape[0]), int(priv_s.shape[1])
        out = torch.empty(T, N, H, dtype=torch.bfloat16, device=self.device)
        for n0 in range(0, N, int(rows_per_pass)):
            part = priv_s[:, n0:n0 + int(rows_per_pass)].contiguous()
            n = int(part.shape[1])
            if part.dtype == torch.float32:
                if part.shape[2] != net.F:
                    raise ValueError("priv_s has %d features, the blueprint takes %d" % (part.shape[2], net.F))
                o16 = net.trunk(part)[0]
            elif part.dtype == torch.bfloat16:
                if part.shape[2] != net.Fp:
                    raise ValueError("priv_s_bf16 has %d columns, the blueprint takes %d (in_dim padded to 64)" % (part.shape[2], net.Fp))
                M = T * n
                x = torch.empty(M, H, dtype=torch.bfloat16, device=self.device)
                gemm_nt(part.view(M, net.Fp), net.W1, M, H, net.Fp, bias=net.b1, out16=x, relu=True)
                for l in range(net.L):
                    gates = torch.empty(M, 4 * H, dtype=torch.float32, device=self.device)
                    gemm_nt(x, net.Wih[l], M, 4 * H, H, bias=net.bg[l], out32=gates)
                    x = lstm_layer_forward(gates.view(T, n, 4 * H), net.Whh[l], None, None, keep_gates=False)[0].view(M, H)
                o16 = x.view(T, n, H)
            else:
                raise ValueError("priv_s must be float32 or bfloat16")
            out[:, n0:n0 + n] = o16
        return out

    def logits(self, o16, out=None):
        """o16 bf16 [M, H] -> float32 [M, NZp] (25 logits per slot, zero padding columns)"""
        from .r2d2 import gemm_nt
        o16 = o16.reshape(-1, self.H)
        M = int(o16.shape[0])
        if out is None:
            out = torch.empty(M, self.NZp, dtype=torch.float32, device=self.device)
        gemm_nt(o16, self.w16, M, self.NZp, self.H, bias=self.b32, out32=out)
        return out

    def _buffers(self, T, B):
        key = (T, B)
        if key not in self._buf:
            d, M = self.device, T * B
            Mp = (M + 63) // 64 * 64
            i32 = lambda: torch.zeros(B, dtype=torch.int32, device=d)      # noqa: E731
            self._buf[key] = dict(
                z=torch.empty(M, self.NZp, dtype=torch.float32, device=d), dz=torch.zeros(Mp, self.NZp, dtype=torch.bfloat16, device=d),
                dzT=torch.zeros(self.NZp, Mp, dtype=torch.bfloat16, device=d), oT=torch.zeros(self.H, Mp, dtype=torch.bfloat16, device=d),
                ws=torch.empty(self.wgrad_split * self.NZp * self.H, dtype=torch.float32, device=d),
                cs=torch.empty(((M + 127) // 128) * self.NZp, dtype=torch.float32, device=d),
                nll=torch.zeros(B, dtype=torch.float32, device=d), nll0=torch.zeros(B, dtype=torch.float32, device=d), cards=i32(), hits=i32(),
                hits0=i32(), bad=i32(), Mp=Mp)
        return self._buf[key]

    def loss(self, batch, weight, compute_grad=True):
        """batch: o16 bf16 [T, B, H] (features), pool int64 [T, B], compat / cards int32 [T, B, hand_size], seq_len float32 [B];
        weight float32 [B].  -> (nll float32 [B], BeliefStats).  compute_grad: d mean_b(weight_b nll_b) / d (weight, bias) is left in
        the gradient buffers for step(): dW by the split-K GEMM over T * B whose slabs are added in order, db by ordered column
        sums -- no float atomics, the same bits run to run."""
        T, B = check_batch(batch, self.hand_size)
        d, M, lib = self.device, T * B, self.lib
        w = torch.as_tensor(weight, device=d).to(torch.float32).contiguous()
        if tuple(w.shape) != (B,):
            raise ValueError("weight must be [%d]; got %s" % (B, tuple(w.shape)))
        k = self._buffers(T, B)
        o16 = batch["o16"].contiguous().view(M, self.H)
        self.logits(o16, k["z"])
        pool, compat, cards, seq_len = (batch[n].contiguous() for n in ("pool", "compat", "cards", "seq_len"))
        _lib.check(lib.hsad_belief_tail(k["z"].data_ptr(), self.NZp, pool.data_ptr(), compat.data_ptr(), cards.data_ptr(), seq_len.data_ptr(),
                                        w.data_ptr(), T, B, self.hand_size, k["nll"].data_ptr(), k["nll0"].data_ptr(), k["cards"].data_ptr(),
                                        k["hits"].data_ptr(), k["hits0"].data_ptr(), k["bad"].data_ptr(),
                                        k["dz"].data_ptr() if compute_grad else None, self.NZp, _s(d)))
        if compute_grad:
            Mp = k["Mp"]
            tr = lambda src, dst: _lib.check(lib.hsad_transpose_bf16(src.data_ptr(), src.shape[0], src.shape[1], src.stride(0),      # noqa: E731
                                                                     dst.data_ptr(), dst.stride(0), _s(d)))
            tr(k["dz"][:M], k["dzT"])      # (columns M .. Mp of both transposes stay zero)
            tr(o16, k["oT"])
            _lib.check(lib.hsad_gemm_nt_bf16_splitk(k["dzT"].data_ptr(), Mp, k["oT"].data_ptr(), Mp, self.NZp, self.H, Mp, self.wgrad_split,
                                                    k["ws"].data_ptr(), self.gw.data_ptr(), self.H, None, _s(d)))
            self.gb.zero_()
            _lib.check(lib.hsad_colsum_acc_ordered(k["dz"].data_ptr(), 1, M, self.NZp, self.NZp, self.gb.data_ptr(), k["cs"].data_ptr(), _s(d)))
        stats = BeliefStats(nll=k["nll"].clone(), nll0=k["nll0"].clone(), cards=k["cards"].clone(), hits=k["hits"].clone(),
                            hits0=k["hits0"].clone(), bad=k["bad"].clone())
        return stats["nll"], stats

    def step(self, beta1=0.9, beta2=0.999):
        """Adam on the gradient loss() left (hsad_adam_step).  grad_clip None: no clipping -- the clip factor would be the one value
        of the update that depends on an atomically summed norm"""
        self.step_count += 1
        clip = 3.0e38 if self.grad_clip is None else float(self.grad_clip)
        _lib.check(self.lib.hsad_adam_step(self.flat.data_ptr(), self.gflat.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.flat.numel(),
                                           clip, self.lr, beta1, beta2, self.eps, self.step_count, self.scratch.data_ptr(), _s(self.device)))
        self.refresh()

    def sample(self, env, viewer, o16_rows, key, seed):
        """o16_rows bf16 [G, H]: the trunk output of viewer[g]'s current observation in game g -> env.determinize_belief under the
        head's logits -> (status, logp)"""
        o16_rows = o16_rows.contiguous()
        if tuple(o16_rows.shape) != (env.G, self.H) or o16_rows.dtype != torch.bfloat16:
            raise ValueError("o16_rows must be bfloat16 [%d, %d]" % (env.G, self.H))
        if env.H != self.hand_size:
            raise ValueError("the env deals hands of %d, the head was made for %d" % (env.H, self.hand_size))
        return env.determinize_belief(viewer, self.logits(o16_rows), key, seed)


def check_state(sd, hand_size=None, H=None):
    """a saved head -> (hand_size, H); ValueError when the dict is no head or not of the expected shape"""
    for k in ("belief.weight", "belief.bias", "hand_size", "H"):
        if k not in sd:
            raise ValueError("not a belief head: no %r" % k)
    hs, h = check_head_args(sd["hand_size"], sd["H"])
    if tuple(sd["belief.weight"].shape) != (TYPES * hs, h) or tuple(sd["belief.bias"].shape) != (TYPES * hs,):
        raise ValueError("belief.weight / belief.bias are %s / %s, hand_size %d and H %d need [%d, %d] / [%d]"
                         % (tuple(sd["belief.weight"].shape), tuple(sd["belief.bias"].shape), hs, h, TYPES * hs, h, TYPES * hs))
    if (hand_size is not None and hs != int(hand_size)) or (H is not None and h != int(H)):
        raise ValueError("the saved head is for hand_size %d, H %d; this one is hand_size %s, H %s" % (hs, h, hand_size, H))
    return hs, h


class BeliefSampler:
    """A head as the searches use it (search.PolicySearch(sampler="learned", belief=...)): belief.weight / belief.bias alone -- no
    blueprint, no trunk, no optimiser state.  The features are the acting agent's own: the top LSTM layer's new h after the root
    act.  head: a BeliefHead (its bf16 operand and bias are shared, so a head that is still being fitted is sampled as it stands),
    a state dict (BeliefHead.state()) or the path of a saved one.  ValueError when the dict is no head (check_state), before the
    device is touched."""

    def __init__(self, head, device="cuda:0"):
        if isinstance(head, BeliefHead):
            self.device, self.lib = head.device, head.lib
            self.hand_size, self.H, self.NZ, self.NZp = head.hand_size, head.H, head.NZ, head.NZp
            self.w16, self.b32 = head.w16, head.b32
        else:
            sd = torch.load(head, map_location="cpu") if isinstance(head, (str, os.PathLike)) else head
            if not isinstance(sd, dict):
                raise ValueError("not a belief head: expected a BeliefHead, its state dict or a saved one; got %s" % type(sd).__name__)
            self.hand_size, self.H = check_state(sd)
            self.NZ, self.NZp = TYPES * self.hand_size, padded_logits(self.hand_size)
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise _lib.HsadError("BeliefSampler needs a ROCm device (got %s); there is no CPU path" % device)
            self.lib = _lib.load_library()
            w32 = torch.zeros(self.NZp, self.H, dtype=torch.float32, device=self.device)
            self.b32 = torch.zeros(self.NZp, dtype=torch.float32, device=self.device)
            w32[:self.NZ].copy_(sd["belief.weight"].to(self.device, torch.float32))
            self.b32[:self.NZ].copy_(sd["belief.bias"].to(self.device, torch.float32))
            self.w16 = torch.zeros(self.NZp, self.H, dtype=torch.bfloat16, device=self.device)
            _lib.check(self.lib.hsad_prepare_weight(w32.data_ptr(), self.NZp, self.H, w32.stride(0), None, self.w16.data_ptr(),
                                                    self.w16.stride(0), None, 0, _s(self.device)))

    def rows(self, h_top, player):
        """h_top float32 [G * P, H] (row g * P + p: the top LSTM layer's h), player int32 [G] -> bfloat16 [G, H]: the row of
        player[g] per game, zeros where it is out of range (hsad_search_belief_rows)"""
        G = int(player.shape[0])
        if (h_top.dtype != torch.float32 or h_top.dim() != 2 or h_top.shape[1] != self.H or h_top.shape[0] % max(G, 1) or not h_top.is_contiguous()
                or G < 1 or player.dtype != torch.int32):
            raise ValueError("h_top must be contiguous float32 [G * P, %d] and player int32 [G]; got %s %s and %s %s"
                             % (self.H, h_top.dtype, tuple(h_top.shape), player.dtype, tuple(player.shape)))
        out = torch.empty(G, self.H, dtype=torch.bfloat16, device=self.device)
        _lib.check(self.lib.hsad_search_belief_rows(h_top.data_ptr(), player.contiguous().data_ptr(), G, int(h_top.shape[0]) // G, self.H,
                                                    out.data_ptr(), out.stride(0), _s(self.device)))
        return out

    def logits(self, h_top, player):
        """-> float32 [G, NZp]: the head's logits for the seat player[g] of every game, from the acting agent's state (rows, then
        the head's GEMM): two launches, once per search call"""
        from .r2d2 import gemm_nt
        o16 = self.rows(h_top, player)
        G = int(o16.shape[0])
        out = torch.empty(G, self.NZp, dtype=torch.float32, device=self.device)
        gemm_nt(o16, self.w16, G, self.NZp, self.H, bias=self.b32, out32=out)
        return out


def belief_batches(data, o16, rows, seed):
    """CloneDataset.batches with the cached trunk features in place of the observations -> (batch for BeliefHead.loss, weight)"""
    if data.pool is None:
        raise ValueError("the dataset carries no hand knowledge (sequences_from_records(..., knowledge=True))")
    for batch, weight, index in data.batches(rows, seed):
        src = index.clamp(min=0)
        yield dict(o16=o16.index_select(1, src), pool=batch["pool"], compat=batch["compat"], cards=batch["cards"], seq_len=batch["seq_len"]), weight


def run_epoch(head, data, o16, rows, seed, train):
    """one pass -> BeliefStats.per_card() over the whole pass; train: one Adam step per batch"""
    tot = torch.zeros(6, dtype=torch.float64, device=data.seq_len.device)
    for batch, weight in belief_batches(data, o16, rows, seed):
        _, st = head.loss(batch, weight, compute_grad=train)
        if train:
            head.step()
        real = weight.double()
        tot += torch.stack([(st["nll"].double() * real).sum(), (st["nll0"].double() * real).sum(), st["cards"].double().sum(),
                            st["hits"].double().sum(), st["hits0"].double().sum(), st["bad"].double().sum()])
    nll, nll0, n, h, h0, bad = tot.tolist()
    if bad:
        raise _lib.HsadError("%d recorded hands are impossible under their own card knowledge" % int(bad))
    n = max(n, 1.0)
    return dict(nll=nll / n, nll0=nll0 / n, top1=h / n, top1_0=h0 / n, cards=int(n))


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="fit a hand-belief head on a blueprint's trunk to recorded games")
    p.add_argument("--blueprint", type=str, default="", help="the weight file whose trunk the head reads")
    p.add_argument("--games", type=str, default="", help="a file of game records (JSON lines, game_record.save)")
    p.add_argument("--teacher", type=str, nargs="+", default=[], help="instead of --games: rule-bot presets or weight files that play the games")
    p.add_argument("--num_game", type=int, default=1000)
    p.add_argument("--seat", type=str, default="", help="only the seats of this name (the records' meta[\"seats\"]), or a seat index")
    p.add_argument("--save_dir", type=str, default="")
    p.add_argument("--seed", type=int, default=10001)
    p.add_argument("--sad", type=int, default=1)
    p.add_argument("--num_player", type=int, default=2)
    p.add_argument("--hand_size", type=int, default=5)
    p.add_argument("--colors", type=int, default=5)
    p.add_argument("--ranks", type=int, default=5)
    p.add_argument("--max_information_tokens", type=int, default=8)
    p.add_argument("--max_life_tokens", type=int, default=3)
    p.add_argument("--eval_bomb", type=int, default=0)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--eps", type=float, default=1e-8)
    p.add_argument("--train_device", type=str, default="cuda:0")
    p.add_argument("--batchsize", type=int, default=128)
    p.add_argument("--num_epoch", type=int, default=10)
    p.add_argument("--max_len", type=int, default=80)
    p.add_argument("--holdout", type=float, default=0.1)
    return p.parse_args(argv)


def main(argv=None):
    from .clone import check_rules, records_from_teacher, sequences_from_records
    from .rulebot import PRESETS
    from .selfplay import game_rules
    args = parse_args(argv)
    dev = args.train_device
    if not args.blueprint:
        raise SystemExit("--blueprint FILE.pthw is needed: the head reads that net's trunk")
    if not os.path.isfile(args.blueprint):
        raise SystemExit("--blueprint %s: no such weight file" % args.blueprint)
    if bool(args.games) + bool(args.teacher) != 1:
        raise SystemExit("give either --games FILE or --teacher NAME")
    if not np.isfinite(args.lr) or args.lr <= 0:
        raise SystemExit("--lr must be finite and positive")
    if not 0.0 < args.holdout < 1.0:
        raise SystemExit("--holdout must lie strictly between 0 and 1")
    if args.games:
        if not os.path.isfile(args.games):
            raise SystemExit("--games %s: no such file" % args.games)
        records = gr.load(args.games)
    else:
        pool = []
        for entry in args.teacher:
            if entry not in PRESETS and not os.path.isfile(entry):
                raise SystemExit("--teacher %s: no rule-bot preset of that name (have: %s) and no weight file" % (entry, ", ".join(sorted(PRESETS))))
            pool.append(PRESETS.get(entry, entry))
        names = [e if e in PRESETS else os.path.basename(e) for e in args.teacher]
        records = records_from_teacher(pool, args.num_game, args.seed, args.sad, num_player=args.num_player, bomb=args.eval_bomb, device=dev,
                                       names=names, hand_size=args.hand_size, **game_rules(args))
    if args.save_dir:
        os.makedirs(args.save_dir, exist_ok=True)
        if args.teacher:
            gr.save(os.path.join(args.save_dir, "games.jsonl"), records)
    r = check_rules(records)
    seats = None if not args.seat else ([int(args.seat)] if args.seat.isdigit() else args.seat)
    head = BeliefHead(args.blueprint, r["hand_size"], dev, lr=args.lr, eps=args.eps)
    data = sequences_from_records(records, args.sad, seats=seats, max_len=args.max_len, device=dev, knowledge=True)
    o16 = head.features(data.priv_s_bf16)      # once: the trunk is frozen
    train, held = data.split(args.holdout, args.seed)      # (by game, each side in the dataset's row order: the features split alike)
    games_held = set(held.game.cpu().tolist())
    is_held = torch.tensor([int(g) in games_held for g in data.game.cpu().tolist()], device=o16.device)
    o_train, o_held = o16[:, ~is_held], o16[:, is_held]
    print("%d games (%d cut at %d moves), %d sequences: %d to fit, %d held out"
          % (len(records), data.truncated, args.max_len, data.n_rows, train.n_rows, held.n_rows), flush=True)
    for epoch in range(args.num_epoch):
        tr = run_epoch(head, train, o_train, args.batchsize, args.seed + epoch, True)
        ho = run_epoch(head, held, o_held, args.batchsize, 0, False)
        print("epoch %d: NLL per card %.4f (exact belief %.4f), top-1 %.4f (exact %.4f); held out: NLL per card %.4f (exact belief %.4f), "
              "top-1 %.4f (exact %.4f)" % (epoch, tr["nll"], tr["nll0"], tr["top1"], tr["top1_0"], ho["nll"], ho["nll0"], ho["top1"], ho["top1_0"]),
              flush=True)
        if args.save_dir:
            head.save(os.path.join(args.save_dir, "belief.pthw"))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
