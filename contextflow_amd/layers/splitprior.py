"""SplitPrior (reference: contextflow/layers/splitprior.py:7-25): second channel half is scored by a
prior and leaves the flow; its log-density is returned as the layer's ldj (B, M)."""
import torch

from .flowlayer import FlowLayer


class SplitPrior(FlowLayer):
    def __init__(self, dist):
        super().__init__()
        self.dist = dist

    def forward(self, x, context=None):
        c = x.shape[1] // 2
        # channel slices are passed to the kernels with their batch stride: no copy
        return x[:, :c], self.dist.log_prob(x[:, c:], context)

    def reverse(self, z, context=None, latent=None, labels=None, temperature=1.0, ctx_draw=False):
        """Inverse by specification: the reference's own line (splitprior.py:18, `self.dist.sample(self.C, ...)`)
        reads an attribute that is never set; the evident intent — resample the split-off half from its prior, one
        draw per batch element, and concatenate — is what runs here.
        latent: the split-off half itself (FlowSequential.encode returns it) is put back instead of a draw.
        labels / temperature (mixture priors): the class-mixture per sample and the scale factor of the draw; the draw and
        the concatenate are then one launch (GaussianMixtureDistribution.draw).
        ctx_draw (FlowSequential.sample under a context): the draw from the mixture with the per-sample shifts of its context net
        (`draw(..., context=)`), the density this layer's forward scores; without it a prior with a context net makes the
        reference's unshifted draw."""
        if latent is not None:
            want = (z.shape[0],) + (tuple(self.dist.size) if hasattr(self.dist, "size") else tuple(z.shape[1:]))
            if tuple(latent.shape) != want or tuple(latent.shape[2:]) != tuple(z.shape[2:]):
                raise ValueError("SplitPrior.reverse: latent of shape %s, this level split off %s" % (tuple(latent.shape), want))
            return torch.cat([z, latent.to(device=z.device, dtype=z.dtype)], dim=1)
        if ctx_draw and hasattr(self.dist, "mG"):
            return self.dist.draw(z.shape[0], labels, temperature, z1=z, context=context if self.dist.context_net else None)
        if labels is not None or temperature != 1.0:
            if not hasattr(self.dist, "mG"):
                raise ValueError("SplitPrior.reverse: labels / temperature need a mixture prior, not %s" % type(self.dist).__name__)
            return self.dist.draw(z.shape[0], labels, temperature, z1=z)
        z2 = (self.dist.sample(z.shape[0], context, need_log_prob=False) if hasattr(self.dist, "mG") else self.dist.sample(z.shape[0], context))[0]
        return torch.cat([z, z2], dim=1)

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]
