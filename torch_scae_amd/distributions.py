"""Gaussian mixture over dim 1 on the HIP kernels (reference:
torch_scae/distributions.py:20-89).

Two flavours share the reference's class name and methods:
  * built with ``make_from_stats`` from arbitrary (materialised) tensors ->
    the generic one-lane-per-pixel mixture kernels;
  * built by ``TemplateBasedImageDecoder`` -> additionally carries the compact
    decoder inputs, and ``log_prob`` takes the fused render+mixture kernel
    (K1) that never reads the (B,K,C,H,W) tensors back from HBM; while those
    tensors are still unrendered (``lazy_render``) and no gradient is wanted,
    ``mode`` / ``mean`` come from the compact inputs too.
"""
import math

import torch

from . import ops


class _NormalView:
    """The slice of torch.distributions.Normal the reference touches
    (``pdf.dist.loc`` / ``.mean`` / ``.scale``)."""

    def __init__(self, loc, scale):
        self._loc = loc            # a tensor, or a thunk that renders it
        self.scale = scale

    @property
    def loc(self):
        if callable(self._loc):
            self._loc = self._loc()
        return self._loc

    @property
    def mean(self):
        return self.loc


class GaussianMixture:
    def __init__(self, normal_dist, mixing_logits, _decoder_inputs=None):
        """
        Args:
          normal_dist: object with ``loc`` [B, K, ...] and ``scale`` (one
            element), e.g. torch.distributions.Normal.
          mixing_logits: tensor [B, K, ...] with K the number of components.
        """
        self.dist = normal_dist
        self._mixing_logits = mixing_logits    # a tensor, or a thunk
        self._decoder_inputs = _decoder_inputs

    @property
    def mixing_logits(self):
        if callable(self._mixing_logits):
            self._mixing_logits = self._mixing_logits()
        return self._mixing_logits

    @property
    def n_components(self):
        if callable(self._mixing_logits) and self._decoder_inputs is not None:
            return self._decoder_inputs.templates.shape[1] + 1
        return self.mixing_logits.shape[1]

    def _sigma(self):
        scale = self.dist.scale
        if not torch.is_tensor(scale):
            scale = torch.tensor([float(scale)], device=self.dist.loc.device)
        if scale.numel() != 1:
            raise ops.ScaeHipError("GaussianMixture kernels take one scalar "
                                   "scale shared by all components")
        return scale

    def mixing_log_prob(self):
        """distributions.py:34-35."""
        return torch.log_softmax(self.mixing_logits, 1)

    def _fused_image(self):
        """True when ``mode()`` / ``mean()`` may come from the fused
        render-and-mode kernel: the mixture was built by the image decoder, its
        rendered tensors have not been made yet (there is nothing to reuse and
        the call leaves them unmade), and no gradient can be asked of the
        result -- the fused kernel is forward only."""
        inputs = self._decoder_inputs
        if inputs is None or not callable(self._mixing_logits) or \
                not callable(getattr(self.dist, "_loc", None)):
            return False
        rendered = getattr(self, "_rendered", None)
        if rendered is not None and rendered.out is not None:
            return False
        return not (torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in inputs.tensors()))

    def mean(self):
        """distributions.py:37-39."""
        if self._fused_image():
            return ops.render_gmm_mode(self._decoder_inputs, mean=True)
        return ops.gmm_mean(self._loc5(), self._ml5()).view(self._out_shape())

    def log_prob(self, x):
        """distributions.py:41-44: logsumexp_K(N(x; loc_k, scale) + log pi_k),
        per pixel and per channel."""
        if self._decoder_inputs is not None and not x.requires_grad:
            return ops.render_gmm_log_prob(self._decoder_inputs, x)
        lp = ops.gmm_log_prob(self._loc5(), self._ml5(), self._sigma(),
                              x.reshape(self._out_shape5()))
        return lp.view(self._out_shape())

    def log_prob_tile_sums(self, x):
        """Partial sums (B, tiles) of ``log_prob(x)`` whose total is
        sum_{b,c,h,w} log_prob -- all the training loss needs -- or None when
        the mixture was not built from compact decoder inputs."""
        if self._decoder_inputs is None or x.requires_grad:
            return None
        return ops.render_gmm_log_prob_sums(self._decoder_inputs, x)

    def mode(self, straight_through_gradient=False, maximum=False):
        """distributions.py:50-77: value of the component with the largest
        mixing log-prob (``maximum``: plus its density at its own mean)."""
        if straight_through_gradient:
            # distributions.py:62-75 with the straight-through estimator: the
            # hard one-hot in the forward value, softmax gradients w.r.t. the
            # mixing coefficients.  A rarely used inspection path: composed
            # from device tensor ops rather than a dedicated kernel.
            mlp = self.mixing_log_prob()
            loc = self.dist.loc
            if maximum:
                sigma = self._sigma().to(loc.dtype)
                extra = (-torch.log(sigma) - 0.5 * math.log(2 * math.pi)) \
                    .expand(loc.shape)       # N(loc; loc, sigma)
                if torch.broadcast_shapes(mlp.shape, extra.shape) != mlp.shape:
                    raise RuntimeError(
                        f"output with shape {list(mlp.shape)} doesn't match "
                        f"the broadcast shape {list(loc.shape)}")
                mlp = mlp + extra
            hard = torch.nn.functional.one_hot(mlp.argmax(1), mlp.shape[1]) \
                .movedim(-1, 1).to(mlp.dtype)
            soft = torch.softmax(mlp, 1)
            mask = (hard - soft).detach() + soft
            return torch.sum(mask * loc, 1)
        if self._fused_image():
            inputs = self._decoder_inputs
            if maximum and inputs.templates_alpha is not None and \
                    inputs.templates.shape[2] > 1:
                # one logit channel for C > 1: the reference's in-place add
                # cannot broadcast (distributions.py:65), as in ops.gmm_mode
                K, (H, W) = inputs.templates.shape[1] + 1, inputs.output_size
                B, C = inputs.pose.shape[0], inputs.templates.shape[2]
                raise RuntimeError(f"output with shape {[B, K, 1, H, W]} "
                                   f"doesn't match the broadcast shape "
                                   f"{[B, K, C, H, W]}")
            scale = self.dist.scale
            if maximum and torch.is_tensor(scale) and scale.numel() != 1:
                # what the materialising route's _sigma() refuses (a non-tensor
                # scale is one number; asking _sigma() for it would render)
                raise ops.ScaeHipError("GaussianMixture kernels take one scalar "
                                       "scale shared by all components")
            # (``maximum`` adds the density of every component at its own mean:
            # one constant under the shared scalar scale, the winner stays)
            return ops.render_gmm_mode(inputs)
        return ops.gmm_mode(self._loc5(), self._ml5(), self._sigma(),
                            maximum).view(self._out_shape())

    # (B, K, C, P) views for the kernels ------------------------------------
    def _loc5(self):
        loc = self.dist.loc
        if loc.dim() < 3:
            raise ops.ScaeHipError("mixture kernels need loc of rank >= 3 "
                                   "(B, K, C, ...)")
        return loc.reshape(loc.shape[0], loc.shape[1], loc.shape[2], -1)

    def _ml5(self):
        ml = self.mixing_logits
        return ml.reshape(ml.shape[0], ml.shape[1], ml.shape[2], -1)

    def _out_shape(self):
        loc = self.dist.loc
        return (loc.shape[0], *loc.shape[2:])

    def _out_shape5(self):
        loc = self.dist.loc
        return (loc.shape[0], loc.shape[2], -1)

    @classmethod
    def make_from_stats(cls, loc, scale, mixing_logits):
        """distributions.py:79-89."""
        return cls(_NormalView(loc, scale), mixing_logits)
