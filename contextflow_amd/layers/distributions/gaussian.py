"""Base densities on the hot path (reference: contextflow/layers/distributions/gaussian.py).

StandardNormal (:10-72) is the Augment noise model; GaussianMixtureDistribution (:118-169) is the
class-conditional prior used by SplitPrior and as the final base density.  The reference broadcasts
(B, M, K, D, H, W); here one register-tiled kernel streams x once per 80 components."""
import math

import torch
import torch.nn as nn

from .. import _derived, _hip, _tape
from ..flowlayer import no_context


class StandardNormal(nn.Module):
    def __init__(self, size, mixtures=1, context_net=None, contextflow=False):
        super().__init__()
        assert mixtures == 1, "mixtures should be 1 in StandardNormal"
        no_context("StandardNormal", context_net)
        self.size = torch.Size(size)
        self.M = mixtures
        self.K = 8
        self.register_buffer("buffer", torch.zeros(1))
        self.context_net = context_net
        self.contextflow = contextflow
        self.fixed_noise = None      # tests inject the reference's captured noise here

    def forward(self, input, context=None):
        return self.log_prob(input, context)

    def log_prob(self, input, context=None):
        """(B,1): sum(-0.5 log 2pi - 0.5 x^2)   gaussian.py:50-54."""
        _hip.require_device(input)
        x, xbs = _hip.bview(input)
        B = x.shape[0]
        N = x.numel() // max(B, 1) if B else 1
        nll = torch.empty(B, device=x.device, dtype=torch.float32)
        _hip.call("cf_std_normal_nll", _hip.p(x), _hip.p(nll), B, N, xbs, _hip.stream())
        return -nll.unsqueeze(-1)

    def sample(self, n_samples, context=None):
        dev = self.buffer.device
        if self.fixed_noise is not None:
            x = self.fixed_noise.to(dev)
        else:
            x = torch.randn(n_samples, *self.size, device=dev, dtype=self.buffer.dtype)
        return x, self.log_prob(x, context)


def gmm_prepare(mG, sG, wG):
    """Per-call parameter transform on the device: a = 1/softplus(sG), nm = -mG, cst (M,K)."""
    M, K = wG.shape
    D = mG.numel() // (M * K)
    dev = mG.device
    a = torch.empty(M * K, D, device=dev, dtype=torch.float32)
    nm = torch.empty(M * K, D, device=dev, dtype=torch.float32)
    cst = torch.empty(M * K, device=dev, dtype=torch.float32)
    _hip.call("cf_gmm_prepare", _hip.p(_hip.f32(mG)), _hip.p(_hip.f32(sG)), _hip.p(_hip.f32(wG)),
              _hip.p(a), _hip.p(nm), _hip.p(cst), M, K, D, _hip.stream())
    return a, nm, cst, M, K, D


def gmm_logprob(x, prepared, out=None, accumulate=False):
    a, nm, cst, M, K, D = prepared
    x, xbs = _hip.bview(x)
    B = x.shape[0]
    assert x.numel() // max(B, 1) == D or B == 0
    if out is None:
        out = torch.empty(B, M, device=x.device, dtype=torch.float32)
        accumulate = False
    nbytes = _hip.lib().cf_gmm_ws_bytes(B, M, K, D)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8) if nbytes else None
    _hip.call("cf_gmm_logprob", _hip.p(x), _hip.p(a), _hip.p(nm), _hip.p(cst), _hip.p(out), _hip.p(ws),
              B, M, K, D, xbs, int(accumulate), _hip.stream())
    return out


GMM_LEVELS_MAX_BATCH = 1024       # below: all mixtures of a flow in one launch pair (the launches are what they cost there)


def gmm_levels_ok(levels):
    """levels: [(x, prepared)].  True when cf_gmm_logprob_levels takes them as they are (no copies made here)."""
    if not 1 <= len(levels) <= 4:
        return False
    M, K = levels[0][1][3], levels[0][1][4]
    if M * K > 256 or not ((16 % K == 0 or M == 1) if M * K <= 16 else 80 % K == 0):
        return False
    for x, (a, nm, cst, m, k, D) in levels:
        xv, xbs = _hip.bview(x)
        if (m, k) != (M, K) or xv is not x or D % 4 or xbs % 4 or (x.data_ptr() | a.data_ptr() | nm.data_ptr()) & 15:
            return False
    return True


def gmm_logprob_levels(levels, ldM=None, ld1=None):
    """logp (B, M) = (ldM +) sum over the levels' mixture log-probs (+ ld1[:, None]) in one launch pair; equals the chain of
    gmm_logprob(..., accumulate=True) + cf_logdet_combine bit for bit.  levels as for gmm_levels_ok (which must hold)."""
    import ctypes
    n = len(levels)
    a0, _, _, M, K, _ = levels[0][1]
    B, dev = levels[0][0].shape[0], levels[0][0].device
    parr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    Ds = (ctypes.c_int * n)(*[lv[1][5] for lv in levels])
    xbs = (ctypes.c_int64 * n)(*[_hip.bview(lv[0])[1] for lv in levels])
    L = _hip.lib()
    ws = torch.empty(max(L.cf_gmm_levels_ws_bytes(n, Ds, B, M, K), 1), device=dev, dtype=torch.uint8)
    out = torch.empty(B, M, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _hip.check(L.cf_gmm_logprob_levels(n, parr([lv[0] for lv in levels]), parr([lv[1][0] for lv in levels]),
                                           parr([lv[1][1] for lv in levels]), parr([lv[1][2] for lv in levels]), Ds, xbs,
                                           _hip.p(ldM), _hip.p(ld1), _hip.p(out), _hip.p(ws), B, M, K, _hip.stream(dev)),
                   "cf_gmm_logprob_levels")
    return out


KEYED_MIN_PER_KEY = 16             # cf_gmm_logprob_keyed from 16 samples per (mean key, scale key) value on average
_bucket_cache = [None, None]
_key_cache = []                    # [(context tensor, signature, key)]: GaussianMixtureDistribution._scale_tables


def _key_buckets(context, key_s, key_m, Us, Um, tag=None, TB=128):
    """Samples grouped by (scale key, mean key) for cf_gmm_logprob_keyed, all on the device (no host sync):
    order (B) int32 = sample indices sorted by key, tiles (T, 4) int32 = [ks, km, first position in order, count] with
    T = ceil(B / TB) + Us Um (an upper bound; unused tiles have count 0).  The last result is kept with the context tensor
    it was made from (the object itself, so its storage cannot be recycled under the cache; in-place writes bump its
    version): the mixtures of all levels of a flow see the same context."""
    sig = (context._version, Us, Um, tag)       # tag: what the keys were formed from (equal tag => equal keys)
    if _bucket_cache[0] is not None and _bucket_cache[0][0] is context and _bucket_cache[0][1] == sig:
        return _bucket_cache[1]
    B, U, dev = key_s.shape[0], Us * Um, key_s.device
    kc = key_s.long() * Um + key_m.long()
    order = torch.argsort(kc).to(torch.int32)
    counts = torch.bincount(kc, minlength=U)
    per = (counts + TB - 1) // TB
    tile_end = torch.cumsum(per, 0)
    row_start = torch.cumsum(counts, 0) - counts
    T = (B + TB - 1) // TB + U
    t = torch.arange(T, device=dev)
    u = torch.searchsorted(tile_end, t, right=True)
    uc = u.clamp(max=U - 1)
    j = t - (tile_end[uc] - per[uc])
    n = torch.where(u < U, (counts[uc] - j * TB).clamp(max=TB), torch.zeros_like(j))
    tiles = torch.stack([uc // Um, uc % Um, row_start[uc] + j * TB, n], 1).to(torch.int32).contiguous()
    _bucket_cache[0], _bucket_cache[1] = (context, sig), (order, tiles)
    return order, tiles


class GaussianDistribution(nn.Module):
    """gaussian.py:75-115: diagonal Gaussian with one (frozen) mean / pre-softplus scale per channel; log_prob (B,) sums
    over (C, H, W).  Evaluated by the mixture kernel with M = K = 1 (the parameters broadcast over the pixels)."""

    def __init__(self, size, mixtures=1, context_net=None, contextflow=False):
        super().__init__()
        assert mixtures == 1, "mixtures should be 1 in GaussianDistribution"
        self.size = size
        self.D = D = size[0]
        self.M = mixtures
        self.m = nn.Parameter(torch.zeros(D, 1, 1), requires_grad=False)
        self.s = nn.Parameter(torch.ones(D, 1, 1), requires_grad=False)
        self.context_net = context_net
        self.contextflow = contextflow

    def forward(self, input, context=None):
        return self.log_prob(input, context)

    def log_prob(self, input, context=None, sum=True):
        _hip.require_device(input, self.m)
        B, C, H, W = input.shape
        mG = _hip.f32(self.m.detach()).expand(C, H, W).contiguous().view(1, 1, C, H, W)
        sG = _hip.f32(self.s.detach()).expand(C, H, W).contiguous().view(1, 1, C, H, W)
        wG = torch.zeros(1, 1, device=input.device, dtype=torch.float32)
        return gmm_logprob(input, gmm_prepare(mG, sG, wG)).view(B)

    def sample(self, n_samples, context=None):
        eps = torch.randn(n_samples, *self.size, device=self.m.device, dtype=torch.float32)
        x = _hip.f32(self.m.detach()) + torch.nn.functional.softplus(_hip.f32(self.s.detach())) * eps
        return x, self.log_prob(x, context)


class _ClassLabels(tuple):
    """(labels tensor | None, label0): checked class labels in the form cf_gmm_draw takes.  A type of its own, so that a user's
    tuple of class indices is never taken for it (GaussianMixtureDistribution._class_labels)."""

    def __new__(cls, tensor, label0):
        return super().__new__(cls, (tensor, label0))


class GaussianMixtureDistribution(nn.Module):
    def __init__(self, size, mixtures=2, components=8, context_net=None, contextflow=False):
        super().__init__()
        self.size = size
        D, H, W = size
        self.D = D
        self.M = M = mixtures
        self.K = K = components
        self.mG = nn.Parameter(torch.randn(M, K, D, H, W))
        self.sG = nn.Parameter(torch.ones(M, K, D, H, W))
        self.wG = nn.Parameter(torch.randn(M, K))
        self.context_net = context_net
        self.contextflow = contextflow
        if self.context_net:                                # gaussian.py:130-137
            self.C = self.context_net.C
            if self.contextflow:
                for p in (self.mG, self.sG, self.wG):
                    p.requires_grad_(False)

    def prepared(self):
        return gmm_prepare(self.mG.detach(), self.sG.detach(), self.wG.detach())

    def _scale_tables(self, context, need_dsig):
        """Table form of the context shifts when the context net is the embedding lookup of model.py:157,162 (CatEmbeddings +
        EyeSampling): the concatenated embedding row is [mean shifts | pre-softplus scale shifts], so each half depends
        only on the context variables whose embedding columns fall in it, i.e. on a key with few values.  Returns
        (key (B) int32, inv_sig, dsig | None, lsum, ckey (B) int32, cm_tab (Um, M*K*D)) or None when the context net is
        anything else (per-sample kernel then)."""
        from ..context import CatEmbeddings, EyeSampling
        cn = self.context_net
        if not (len(cn) == 2 and isinstance(cn[0], CatEmbeddings) and isinstance(cn[1], EyeSampling)):
            return None
        embs = list(cn[0]._embeddings)
        D, H, W = self.size
        half, dE = self.M * self.K * D, embs[0].embedding_dim
        if dE * len(embs) != 2 * half:
            return None

        def keyed(rel):                       # mixed-radix key over the relevant variables, and the grid of all its values
            U, strides = 1, {}
            for i in reversed(rel):
                strides[i] = U
                U *= embs[i].num_embeddings
            return U, strides
        rel_s = [i for i in range(len(embs)) if (i + 1) * dE > half]        # variables that reach the scale half
        rel_m = [i for i in range(len(embs)) if i * dE < half]              # ... the mean half
        Us, st_s = keyed(rel_s)
        Um, st_m = keyed(rel_m)
        if Us * half * H * W * 4 > (256 << 20) or Um * half * 4 > (256 << 20):
            return None
        dev = self.sG.device
        # (storage, version) of every tensor the tables are built from; writes through `.data` bump no version counter:
        # callers that do that (none in this package) must drop the entry themselves (FlowSequential.invalidate_caches)
        def build():
            def rows(U, rel, strides):
                grid = torch.zeros(U, len(embs), dtype=torch.long, device=dev)
                u = torch.arange(U, device=dev)
                for i in rel:
                    grid[:, i] = (u // strides[i]) % embs[i].num_embeddings
                return cn[0](grid)[0]
            cs_tab = _hip.f32(rows(Us, rel_s, st_s)[:, half:])
            cm_tab = _hip.f32(rows(Um, rel_m, st_m)[:, :half])
            inv = torch.empty(Us, half * H * W, device=dev, dtype=torch.float32)
            dsig = torch.empty_like(inv) if need_dsig else None
            lsum = torch.empty(Us, self.M * self.K, device=dev, dtype=torch.float32)
            _hip.call("cf_gmm_ctx_tables", _hip.p(_hip.f32(self.sG.detach())), _hip.p(cs_tab), _hip.p(inv), _hip.p(dsig),
                      _hip.p(lsum), Us, self.M * self.K, D, H * W, _hip.stream())
            return inv, dsig, lsum, cm_tab
        inv, dsig, lsum, cm_tab = _derived.get(self, "tab", _derived.key([self.sG] + [e.weight for e in embs], need_dsig, str(dev)),
                                               build, dev)
        ctx = context.to(device=dev, dtype=torch.long)

        def key_of(rel, strides):
            # the mixtures of all levels of a flow see the same context and, with model.py's embedding widths, form the same keys:
            # kept with the context tensor they were made from (the object itself: its storage cannot be recycled under the cache;
            # in-place writes bump its version) - 11 tiny launches per mixture and call otherwise
            sig = (context._version, tuple(rel), tuple(sorted(strides.items())), tuple(embs[i].num_embeddings for i in rel), str(dev))
            for ent in _key_cache:
                if ent[0] is context and ent[1] == sig:
                    return ent[2]
            key = torch.zeros(ctx.shape[0], dtype=torch.long, device=dev)
            for i in rel:        # clamped: an out-of-range code must not index past the tables (the lookup would raise)
                key += ctx[:, i].clamp(0, embs[i].num_embeddings - 1) * strides[i]
            key = key.to(torch.int32)
            _key_cache.append((context, sig, key))
            del _key_cache[:-4]               # the two keys of the current context (+ those of the one before)
            return key
        return key_of(rel_s, st_s), inv, dsig, lsum, key_of(rel_m, st_m), cm_tab

    def _keyed_tables(self, tab, logw):
        """Per-key parameter rows of cf_gmm_logprob_keyed, kept as long as the scale tables `tab` they belong to: nm (Um, M*K*N) =
        -(mG + mean shift) - the reference's `self.mG + cond_mean` rounded once (gaussian.py:143) - and cst (Us, M*K)."""
        def build():
            D, H, W = self.size
            MK = self.M * self.K
            nm = -(_hip.f32(self.mG.detach()).view(1, MK, D, H * W) + tab[5].view(-1, MK, D, 1))
            cst = logw.reshape(1, MK) - tab[3] - 0.5 * D * H * W * math.log(2 * math.pi)
            return tab[1], nm.reshape(nm.shape[0], -1).contiguous(), cst.contiguous()     # (tab[1] is held: its id stays taken)
        return _derived.get(self, "keyed", (id(tab[1]),), build, tab[1].device)[1:]

    def _log_prob_ctx(self, input, context, tape=None):
        """gaussian.py:146-158: per-sample shifts (B, 2, M, K, D) of the component means / pre-softplus scales."""
        if isinstance(context, list):
            context = context[0]
        x, xbs = _hip.bview(input)
        B, D, H, W = x.shape
        M, K = self.M, self.K
        logw = torch.log_softmax(_hip.f32(self.wG.detach()), dim=-1).contiguous()
        out = torch.empty(B, M, device=x.device, dtype=torch.float32)
        tab = self._scale_tables(context, tape is not None)
        if tab is not None and tape is None:
            # evaluation with the embedding-lookup context net: both halves of the shift come from tables indexed by a
            # key per sample - the (B, 2 M K D) rows of embeddings are never gathered (logp_c of the lookup is 0)
            key, inv, _, lsum, ckey, cm_tab = tab
            Um, Us = cm_tab.shape[0], inv.shape[0]
            N = D * H * W
            if (B >= KEYED_MIN_PER_KEY * Um * Us and 16 < M * K <= 256 and 80 % K == 0 and N % 4 == 0 and xbs % 4 == 0
                    and x.data_ptr() % 16 == 0):
                # saturating batches: samples bucketed by (scale key, mean key) - a workgroup's 128 samples then share their
                # parameter rows and the register-tiled mixture kernel applies (cf_gmm_logprob_keyed)
                nm_tab, cst_tab = self._keyed_tables(tab, logw)
                order, tiles = _key_buckets(context, key, ckey, Us, Um, tuple(e.num_embeddings for e in self.context_net[0]._embeddings))
                T = tiles.shape[0]
                ws = torch.empty(_hip.lib().cf_gmm_keyed_ws_bytes(T, B, M, K, N), device=x.device, dtype=torch.uint8)
                _hip.call("cf_gmm_logprob_keyed", _hip.p(x), _hip.p(inv), _hip.p(nm_tab), _hip.p(cst_tab), _hip.p(key),
                          _hip.p(tiles), _hip.p(order), _hip.p(out), _hip.p(ws), T, B, M, K, N, xbs, 0, _hip.stream())
                return out
            _hip.call("cf_gmm_ctx_logprob_tab", _hip.p(x), _hip.p(_hip.f32(self.mG.detach())), _hip.p(inv), _hip.p(lsum),
                      _hip.p(logw), _hip.p(cm_tab), _hip.p(ckey), _hip.p(key), _hip.p(out), None, B, M, K, D, H * W, xbs, 0,
                      _hip.stream())
            return out
        c, logp_c = self.context_net(context)
        # training: keep the per-component log-joints for the backward (it then skips their recompute)
        lp = torch.empty(B, M * K, device=x.device, dtype=torch.float32) if tape is not None else None
        if tab is not None:
            key, inv, dsig, lsum = tab[:4]
            _hip.call("cf_gmm_ctx_logprob_tab", _hip.p(x), _hip.p(_hip.f32(self.mG.detach())), _hip.p(inv), _hip.p(lsum),
                      _hip.p(logw), _hip.p(_hip.f32(c)), None, _hip.p(key), _hip.p(out), _hip.p(lp), B, M, K, D, H * W, xbs, 0,
                      _hip.stream())
            tab = tab[:4]
        else:
            _hip.call("cf_gmm_ctx_logprob", _hip.p(x), _hip.p(_hip.f32(self.mG.detach())), _hip.p(_hip.f32(self.sG.detach())),
                      _hip.p(logw), _hip.p(_hip.f32(c)), _hip.p(out), _hip.p(lp), B, M, K, D, H * W, xbs, 0, _hip.stream())
        if tape is not None:
            tape.append(_tape.CtxMixture(self, x, _hip.f32(c), logw, context, lp, tab))
        return out + (logp_c * float(H * W)).unsqueeze(-1)

    def log_prob(self, input, context=None):
        """(B, M) class-mixture log-densities   gaussian.py:142-161."""
        _hip.require_device(input, self.mG)
        if self.context_net:
            return self._log_prob_ctx(input, context)
        return gmm_logprob(input, self.prepared())

    def component_cdf(self):
        """(M, K) float32: cumulative component weights of every class-mixture, the table cf_gmm_draw picks the component from
        (the first k with u < cdf[m, k]).  softmax(wG, -1) and its running sum in fp64, rounded once; the last column is
        exactly 1, so every u in [0, 1) finds its component.  Kept while wG is unchanged (layers/_derived.py); lives where
        wG lives, a host tensor included."""
        wG = self.wG.detach()

        def build():
            cdf = torch.cumsum(torch.softmax(wG.double(), dim=-1), dim=-1).to(torch.float32)
            cdf[:, -1] = 1.0
            return cdf.contiguous()
        return _derived.get(self, "cdf", _derived.key([self.wG], str(wG.device)), build, wG.device)

    def _class_labels(self, labels, n_samples):
        """`labels` of `sample` in the form cf_gmm_draw takes, a _ClassLabels: (None, m) for one class-mixture m for every sample, or
        ((n,) int32 tensor on the device, 0).  An int, a sequence (list, tuple, ...) or a host tensor is checked here - ValueError for
        a value outside [0, M) or a length other than n; a device tensor is only checked for its length (no host sync): the
        kernel clamps its values as the keyed mixture kernels clamp their keys (a 0-dim device tensor is that class for every
        sample).  None: class-mixture 1, the reference's hard-coded `x[:, 1]` (0 when M == 1).  A _ClassLabels (what
        FlowSequential.sample prepared once for every level) is returned as it is."""
        M = self.M
        if isinstance(labels, _ClassLabels):
            return labels
        if labels is None:
            return _ClassLabels(None, 1 if M > 1 else 0)
        try:
            t = labels if torch.is_tensor(labels) else torch.as_tensor(labels)
        except (TypeError, RuntimeError, ValueError) as e:
            raise ValueError("labels: an int or a sequence / tensor of integer class indices expected (%s)" % e) from None
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("labels: integer class indices expected, got %s" % t.dtype)
        if t.dim() == 0 and not t.is_cuda:
            m = int(t)
            if not 0 <= m < M:
                raise ValueError("labels: class %d outside [0, %d)" % (m, M))
            return _ClassLabels(None, m)
        if t.dim() == 0:
            t = t.reshape(1).expand(n_samples)
        if t.dim() != 1 or t.shape[0] != n_samples:
            raise ValueError("labels: shape %s for %d samples" % (tuple(t.shape), n_samples))
        if not t.is_cuda and t.numel() and not (0 <= int(t.min()) and int(t.max()) < M):
            raise ValueError("labels: values outside [0, %d)" % M)
        return _ClassLabels(t.to(device=self.mG.device, dtype=torch.int32).contiguous(), 0)

    def draw(self, n_samples, labels=None, temperature=1.0, z1=None, context=None):
        """One cf_gmm_draw launch: per sample the class-mixture of `labels` (see _class_labels), a component by its weight,
        mG + temperature * softplus(sG) * eps - noise from the in-kernel Philox stream, positioned by torch's CUDA generator
        (`_hip.noise_nonce`) - written behind the channels of z1 (B, C1, H, W), if given: the draw and the concatenate of
        SplitPrior.reverse in one pass.  Returns (n, C1 + C, H, W).
        A prior with a context net takes `context` ((n, nctx) integers): the rows of shifts c = context_net(context) (B, 2 M K C) are
        gathered and cf_gmm_ctx_draw draws from (mG + cm_b) + temperature * softplus(sG + cs_b) * eps - the density `log_prob(.,
        context)` scores (the reference's own `sample` ignores the shifts: `sample` below keeps that behaviour)."""
        _hip.require_device(self.mG, z1)
        if self.context_net and context is None:
            raise ValueError("draw: a mixture with a context net needs its context")
        temperature = float(temperature)
        if not (temperature >= 0.0 and math.isfinite(temperature)):
            raise ValueError("temperature must be finite and >= 0, got %r" % temperature)
        dev = self.mG.device
        lab, label0 = self._class_labels(labels, n_samples)
        C, H, W = self.mG.shape[2:]
        D = C * H * W
        C1, D1, zbs = 0, 0, 0
        if z1 is not None:
            z1, zbs = _hip.bview(z1)
            if z1.dim() != 4 or z1.shape[0] != n_samples or tuple(z1.shape[2:]) != (H, W):
                raise ValueError("draw: kept half of shape %s for %d samples of a prior over %s" % (tuple(z1.shape), n_samples, (C, H, W)))
            C1 = z1.shape[1]
            D1 = C1 * H * W
        shifts = None
        if self.context_net:
            if isinstance(context, list):
                context = context[0]
            if context.shape[0] != n_samples:
                raise ValueError("draw: a context of %d rows for %d samples" % (context.shape[0], n_samples))
            shifts = _hip.f32(self.context_net(context)[0])
            if tuple(shifts.shape) != (n_samples, 2 * self.M * self.K * C):
                raise ValueError("draw: context net output of shape %s, (%d, %d) expected" % (tuple(shifts.shape), n_samples, 2 * self.M * self.K * C))
        key, nonce = _hip.noise_nonce(dev)
        out = torch.empty(n_samples, C1 + C, H, W, device=dev, dtype=torch.float32)
        if shifts is not None:
            _hip.call("cf_gmm_ctx_draw", _hip.p(_hip.f32(self.mG.detach())), _hip.p(_hip.f32(self.sG.detach())), _hip.p(self.component_cdf()),
                      _hip.p(shifts), _hip.p(lab), label0, None, None, _hip.p(nonce), key, _hip.p(z1 if D1 else None), zbs, D1, _hip.p(out),
                      n_samples, self.M, self.K, D, H * W, temperature, _hip.stream())
            return out
        _hip.call("cf_gmm_draw", _hip.p(_hip.f32(self.mG.detach())), _hip.p(_hip.f32(self.sG.detach())), _hip.p(self.component_cdf()),
                  _hip.p(lab), label0, None, None, _hip.p(nonce), key, _hip.p(z1 if D1 else None), zbs, D1, _hip.p(out), n_samples,
                  self.M, self.K, D, temperature, _hip.stream())
        return out

    def sample(self, n_samples, context=None, need_log_prob=True, *, labels=None, temperature=1.0):
        """gaussian.py:163-169: draw from the mixture of class-mixture index 1 (the reference hard-codes `x[:, 1]`;
        with a single mixture, where the reference raises, index 0 is used) and return (x, log_prob(x)).
        labels (an int, or n class indices) / temperature (the components' scales are multiplied by it): the draw of
        `draw` instead - any class-mixture, per sample; with both left at their defaults the reference's draw above runs,
        in its torch.multinomial / torch.randn order."""
        if labels is not None or temperature != 1.0:
            x = self.draw(n_samples, labels, temperature)
            return x, (self.log_prob(x, context) if need_log_prob else None)
        _hip.require_device(self.mG)
        dev = self.mG.device
        m = 1 if self.M > 1 else 0
        w = torch.softmax(self.wG.detach()[m].float(), dim=-1)
        k = torch.multinomial(w, n_samples, replacement=True)              # component per sample (RNG: plumbing)
        rows = (m * self.K + k).to(torch.int64).contiguous()
        D = self.mG[0, 0].numel()
        eps = torch.randn(n_samples, D, device=dev, dtype=torch.float32)
        x = torch.empty(n_samples, *self.mG.shape[2:], device=dev, dtype=torch.float32)
        _hip.call("cf_gmm_sample", _hip.p(_hip.f32(self.mG.detach())), _hip.p(_hip.f32(self.sG.detach())), _hip.p(rows),
                  _hip.p(eps), _hip.p(x), n_samples, D, _hip.stream())
        return x, (self.log_prob(x, context) if need_log_prob else None)
