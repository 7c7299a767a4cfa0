"""PyG 1.4.2 ``torch_geometric.nn.models.autoencoder`` on the MI355X: the decoder and the loss that close a link-prediction step::

    model = npi.GAE(encoder)                                   # decoder: npi.InnerProductDecoder()
    z = model.encode(x, edge_index)                            # a tensor [N, F], or a pair (z_src, z_dst) from bipartite layers
    loss = model.recon_loss(z, pos_edge_index)                 # negatives drawn on the device, as many as positives
    loss.backward()
    loss = model.ranking_loss(z, pos_edge_index, num_neg=8, loss="softmax")   # each positive against 8 corrupted targets of its source
    auc, ap = model.test(z, pos_edge_index, neg_edge_index)    # 0-d float64 device tensors: float(auc) is PyG's number
    prob, ids = model.predict(z, k, pos_edge_index)            # [R, k] each: the k most likely NEW links of every source row
    m = model.test_ranking(z, test_edge_index, pos_edge_index)  # filtered MRR / mean rank / Hits@K of held-out links

    model = npi.VGAE(encoder, seed=0)                          # the encoder returns (mu, logvar)
    z = model.encode(x, edge_index)                            # training mode: mu + eps * exp(0.5 * logvar), eps seeded (Rule N)
    loss = model.recon_loss(z, pos_edge_index) + model.kl_loss() / num_nodes

``InnerProductDecoder.forward`` is ``functional.pair_scores`` (one launch over the pair list, no sort), ``GAE.recon_loss`` is
``functional.link_loss`` (one forward launch, no logits written; the backward is the layers' own aggregation: no float atomics,
bitwise reproducible), ``GAE.test`` is ``rank.rank_metrics`` (ROC-AUC and average precision of the decoder's outputs: one device
sort, no copy to the host).  ``GAE.ranking_loss`` is ``functional.ranking_loss`` (BPR, a margin hinge or the sampled
softmax of every positive against its own corrupted targets: one forward launch, the same backward).
``InnerProductDecoder.forward_all`` -- the dense ``[N, N]`` product -- is not provided:
``InnerProductDecoder.topk`` / ``GAE.predict`` (``topk.topk_links``) give each row's best ``k`` of it without the matrix, and
``InnerProductDecoder.ranks`` / ``GAE.test_ranking`` (``link_rank.link_ranks``) the rank of a held-out link within it.
``VGAE.encode`` is ``functional.reparametrize_kl``: the sample and the KL term from one launch, the noise a pure function of ``(seed,
draw, tick, table, row, column)`` that the backward recomputes, so a VGAE step is as reproducible as a GAE step.  ``ARGA`` / ``ARGVA``
add PyG's adversarial regulariser as torch compositions over the user's discriminator.
CPU tensors raise ``NpiError``: there is no CPU path.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import functional as F_
from .negative import NegativeSampler
from .rank import rank_metrics
from .link_rank import link_ranks, ranking_metrics
from .softmax_link import listwise_loss
from .topk import topk_links


def _reset(module) -> None:
    """PyG ``inits.reset``: ``reset_parameters()`` of the module, or of each of its children"""
    if module is None:
        return
    if hasattr(module, "reset_parameters"):
        module.reset_parameters()
    else:
        for child in (module.children() if hasattr(module, "children") else []):
            _reset(child)


class InnerProductDecoder(nn.Module):
    """``forward(z, edge_index, sigmoid=True)``: ``sigmoid(<z_src[edge_index[0]], z_dst[edge_index[1]]>)`` per pair, ``[M]``;
    ``sigmoid=False``: the logits.  ``z``: a tensor (one id space) or a pair ``(z_src, z_dst)``; ``edge_index``: the ``[2, M]``
    LongTensor or a ``BipartiteGraph`` of it (``functional.pair_scores``)."""

    def forward(self, z, edge_index, sigmoid: bool = True) -> torch.Tensor:
        value = F_.pair_scores(z, edge_index)
        return torch.sigmoid(value) if sigmoid else value

    def group_scores(self, z, pos_edge_index: torch.Tensor, neg_dst: torch.Tensor, sigmoid: bool = False) -> torch.Tensor:
        """``functional.group_scores(z, pos_edge_index, neg_dst)``: ``[P, 1 + K]``, column 0 the positive's logit, column ``c`` that
        of ``(pos_edge_index[0, p], neg_dst[p, c - 1])``; an empty (``-1``) slot holds ``-inf`` (``sigmoid=True``: probability 0)."""
        value = F_.group_scores(z, pos_edge_index, neg_dst)
        return torch.sigmoid(value) if sigmoid else value

    def topk(self, z, k: int, exclude=None, rows: Optional[torch.Tensor] = None, sigmoid: bool = True):
        """``(scores, ids)`` of ``topk.topk_links(z, k, exclude, rows)``: per query row the ``k`` best targets that ``exclude`` does
        not hold, ``[R, k]`` each, the scores through ``torch.sigmoid`` as in ``forward`` (``sigmoid=False``: the logits; a slot
        without a candidate holds id ``-1`` and logit ``-inf``, probability 0).  What ``forward_all`` followed by a mask and
        ``torch.topk`` would give, without the ``[N, N]`` matrix."""
        value, ids = topk_links(z, k, exclude=exclude, rows=rows)
        return (torch.sigmoid(value) if sigmoid else value), ids

    def ranks(self, z, edge_index: torch.Tensor, exclude=None):
        """``link_rank.link_ranks(z, edge_index, exclude)``: for every pair of ``edge_index [2, Q]`` the counts of the targets that
        ``exclude`` does not hold and that score above, or equal to, the pair's own target (a ``LinkRanks``; ``score`` holds the
        logits) -- what ``forward_all``, a mask and a compare-and-sum would give, without the ``[N, N]`` matrix."""
        return link_ranks(z, edge_index, exclude=exclude)


class GAE(nn.Module):
    """``GAE(encoder, decoder=None)``: ``encode`` runs the encoder, ``decode`` the decoder (default ``InnerProductDecoder``),
    ``recon_loss`` the link-prediction loss of embeddings ``z``.  ``draw`` counts the negative draws ``recon_loss`` has made
    (readable and settable, like ``NegativeSampler.draw``): successive calls see different negatives, and a run that starts from the
    same ``seed`` and ``draw`` sees the same ones."""

    def __init__(self, encoder, decoder=None):
        super().__init__()
        self.encoder = encoder
        self.decoder = InnerProductDecoder() if decoder is None else decoder
        self.draw = 0
        GAE.reset_parameters(self)

    def reset_parameters(self) -> None:
        _reset(self.encoder)
        _reset(self.decoder)

    def encode(self, *args, **kwargs):
        return self.encoder(*args, **kwargs)

    def decode(self, *args, **kwargs):
        return self.decoder(*args, **kwargs)

    def recon_loss(self, z, pos_edge_index: torch.Tensor, neg_edge_index: Optional[torch.Tensor] = None, loss: str = "gae",
                   seed: int = 0) -> torch.Tensor:
        """PyG's ``recon_loss(z, pos_edge_index)`` (``loss="gae"``; ``"bce"``: ``binary_cross_entropy_with_logits`` over all
        pairs), computed by ``functional.link_loss`` whatever the decoder.  ``neg_edge_index=None`` draws as many negatives as
        there are positives (``NegativeSampler(pos_edge_index, size, seed).pairs(draw=self.draw)``, then ``draw`` counts up): one
        id space excludes ``(v, v)`` -- PyG's "do not include self-loops in negative samples" --, a pair ``z`` draws from
        ``size = (n_src, n_dst)``."""
        if neg_edge_index is None:
            z_src, z_dst, n_src, n_dst = F_._pair_tables(z, None, "GAE.recon_loss")
            if loss not in F_.PAIR_LOSSES:
                raise ValueError(f"GAE.recon_loss: loss is 'gae' or 'bce', got {loss!r}")
            one = z_dst is None
            sampler = NegativeSampler(pos_edge_index, n_src if one else (n_src, n_dst), seed=seed, allow_loops=not one)
            neg_edge_index = sampler.pairs(draw=self.draw)
            self.draw += 1
        return F_.link_loss(z, pos_edge_index, neg_edge_index, loss=loss)

    def ranking_loss(self, z, pos_edge_index: torch.Tensor, num_neg: int = 1, loss: str = "bpr", margin: float = 1.0,
                     scale: float = 1.0, known_edge_index: Optional[torch.Tensor] = None, neg_dst: Optional[torch.Tensor] = None,
                     seed: int = 0) -> torch.Tensor:
        """``functional.ranking_loss`` of every positive against ``num_neg`` corrupted targets of its own source (``loss``: ``"bpr"``,
        ``"margin"`` or ``"softmax"``) -- the objective ``test_ranking`` and ``predict`` measure, where ``recon_loss`` is
        pointwise.  ``neg_dst=None`` draws them: ``NegativeSampler(known_edge_index, size, seed).corrupt(...)`` (Rule T; targets the
        source has no edge to in ``known_edge_index``, default ``pos_edge_index``; Rule T knows no loop exclusion) under draw
        ``self.draw``, which then counts up as in ``recon_loss``.  ``neg_dst [P, K]``: the corrupted targets themselves, e.g. the
        ids of ``predict`` as hard negatives (``num_neg`` is then not read; no draw is taken)."""
        if neg_dst is None:
            z_src, z_dst, n_src, n_dst = F_._pair_tables(z, None, "GAE.ranking_loss")
            if loss not in F_.GROUP_LOSSES:
                raise ValueError(f"GAE.ranking_loss: loss is 'bpr', 'margin' or 'softmax', got {loss!r}")
            num_neg = int(num_neg)
            if num_neg < 0 or num_neg > F_.GROUP_MAX_K:
                raise ValueError(f"GAE.ranking_loss: num_neg must lie in [0, {F_.GROUP_MAX_K}], got {num_neg}")
            if (not isinstance(pos_edge_index, torch.Tensor) or pos_edge_index.dtype != torch.int64 or pos_edge_index.dim() != 2
                    or pos_edge_index.size(0) != 2):
                raise ValueError("GAE.ranking_loss: pos_edge_index must be a LongTensor of shape [2, P]")
            one = z_dst is None
            known = pos_edge_index if known_edge_index is None else known_edge_index
            sampler = NegativeSampler(known, n_src if one else (n_src, n_dst), seed=seed, allow_loops=not one)
            P = int(pos_edge_index.size(1))
            neg_dst = sampler.corrupt(pos_edge_index[0].repeat_interleave(num_neg), draw=self.draw).view(P, num_neg)
            self.draw += 1
        return F_.ranking_loss(z, pos_edge_index, neg_dst, loss=loss, margin=margin, scale=scale)

    def listwise_loss(self, z, pos_edge_index: torch.Tensor, known_edge_index=None, scale: float = 1.0) -> torch.Tensor:
        """``softmax_link.listwise_loss``: every positive against ALL targets its source has no edge to in ``known_edge_index`` (the
        ``[2, E]`` LongTensor, or a ``KnownLinks`` of it built once; default: ``pos_edge_index`` itself) -- the full-softmax
        objective whose optimum ``test_ranking`` measures, where ``ranking_loss`` samples ``num_neg`` corruptions.  The target is
        always in its own denominator; ``(v, v)`` is no candidate when ``z`` is one id space, as in ``predict`` and
        ``test_ranking``.  The inner product is scored whatever the decoder."""
        one = isinstance(z, torch.Tensor) or (isinstance(z, (tuple, list)) and len(z) == 2 and z[0] is z[1])
        known = pos_edge_index if known_edge_index is None else known_edge_index
        return listwise_loss(z, pos_edge_index, exclude=known, scale=scale, allow_loops=not one)

    def test(self, z, pos_edge_index: torch.Tensor, neg_edge_index: torch.Tensor):
        """PyG's ``test(z, pos_edge_index, neg_edge_index)``: ``(auc, ap)`` = ``roc_auc_score`` and ``average_precision_score`` of
        ``decode(z, ., sigmoid=True)`` over ``cat([pos, neg])`` with the positives labelled 1 -- ``rank.rank_metrics`` in its
        ``n_pos`` form, so both are 0-d float64 DEVICE tensors and nothing is read back (``float(auc)`` is the number PyG returns).
        The float32 sigmoid outputs are what is ranked, as in PyG: where the sigmoid saturates, its ties are PyG's ties."""
        with torch.no_grad():
            pos_pred = self.decode(z, pos_edge_index, sigmoid=True)
            neg_pred = self.decode(z, neg_edge_index, sigmoid=True)
            return rank_metrics(torch.cat([pos_pred, neg_pred]), n_pos=int(pos_pred.numel()))

    def predict(self, z, k: int, known_edge_index, rows: Optional[torch.Tensor] = None, sigmoid: bool = True):
        """The ``k`` most likely NEW links of every query row (``rows``: None, every source): ``(scores, ids)``, ``[R, k]`` each, by
        ``topk.topk_links`` with ``known_edge_index`` (the ``[2, E]`` LongTensor, or a ``KnownLinks`` of it built once) excluded --
        and ``(v, v)`` too when ``z`` is one id space, as ``recon_loss`` draws no such negative.  Scores through ``torch.sigmoid``
        unless ``sigmoid=False``.  The inner product is scored whatever the decoder, as in ``recon_loss``."""
        one = isinstance(z, torch.Tensor) or (isinstance(z, (tuple, list)) and len(z) == 2 and z[0] is z[1])
        value, ids = topk_links(z, k, exclude=known_edge_index, rows=rows, allow_loops=not one)
        return (torch.sigmoid(value) if sigmoid else value), ids

    def test_ranking(self, z, pos_edge_index: torch.Tensor, known_edge_index, ks=(1, 3, 10), ties: str = "average"):
        """The filtered ranking metrics of the held-out links ``pos_edge_index``: ``{"mrr", "mean_rank", "hits@k" ...}`` (0-d float64
        device tensors) by ``link_rank.ranking_metrics`` -- every positive ranked against all targets its source has no edge to in
        ``known_edge_index`` (the ``[2, E]`` LongTensor, or a ``KnownLinks`` of it built once), and never against ``(v, v)`` when
        ``z`` is one id space, as in ``predict``.  Where ``test`` compares with sampled negatives, this says whether ``predict(z,
        k, ...)`` shows the true partner within its ``k`` slots.  The inner product is scored whatever the decoder."""
        one = isinstance(z, torch.Tensor) or (isinstance(z, (tuple, list)) and len(z) == 2 and z[0] is z[1])
        return ranking_metrics(z, pos_edge_index, exclude=known_edge_index, ks=ks, ties=ties, allow_loops=not one)


MAX_LOGVAR = 10
EPS = 1e-15


def _is_pair(t) -> bool:
    return isinstance(t, (tuple, list)) and len(t) == 2


class VGAE(GAE):
    """PyG 1.4.2 ``VGAE(encoder, decoder=None)``; the encoder returns ``(mu, logvar)`` -- or, from bipartite layers,
    ``((mu_src, logvar_src), (mu_dst, logvar_dst))``.  ``seed`` and the counter ``draw_noise`` (readable and settable; separate from
    ``draw``, the negatives' counter) name the noise of a training-mode ``encode``: successive calls draw differently, and a run that
    starts from the same ``seed`` and ``draw_noise`` repeats bit for bit.  ``tick``: the device word of ``functional.GaussianNoise``,
    for fresh noise on every replay of a captured step.  Everything of ``GAE`` works on the result."""

    def __init__(self, encoder, decoder=None, seed: int = 0, tick: Optional[torch.Tensor] = None):
        super().__init__(encoder, decoder)
        F_.GaussianNoise(seed, 0, tick)                        # the argument checks
        self.seed, self.tick, self.draw_noise = seed, tick, 0
        self.__mu__ = self.__logvar__ = self.__kl__ = None

    def reparametrize(self, mu, logvar):
        """``mu + eps * exp(0.5 * min(logvar, MAX_LOGVAR))`` in training mode -- under draw ``draw_noise``, which then counts up --
        and ``mu`` in evaluation.  ``mu`` / ``logvar``: tensors, or pairs ``(mu_src, mu_dst)`` / ``(logvar_src, logvar_dst)`` (tables
        0 and 1 of the rule).  The KL term of the same launch is kept for ``kl_loss()``."""
        if not self.training:
            self.__kl__ = None
            return mu
        rule = F_.GaussianNoise(self.seed, self.draw_noise, self.tick)
        self.draw_noise += 1
        if _is_pair(mu):
            n_total = int(mu[0].size(0)) + int(mu[1].size(0))
            z_src, kl_src = F_.reparametrize_kl(mu[0], logvar[0], rule, table=0, n_total=n_total, max_logvar=MAX_LOGVAR)
            z_dst, kl_dst = F_.reparametrize_kl(mu[1], logvar[1], rule, table=1, n_total=n_total, max_logvar=MAX_LOGVAR)
            self.__kl__ = kl_src + kl_dst
            return z_src, z_dst
        z, self.__kl__ = F_.reparametrize_kl(mu, logvar, rule, max_logvar=MAX_LOGVAR)
        return z

    def encode(self, *args, **kwargs):
        """runs the encoder, keeps its ``__mu__`` and ``__logvar__`` (as the encoder returned them: the clamp at ``MAX_LOGVAR``
        happens inside the kernels) and returns ``reparametrize`` of them"""
        out = self.encoder(*args, **kwargs)
        if not _is_pair(out):
            raise TypeError("VGAE: the encoder returns (mu, logvar), or ((mu_src, logvar_src), (mu_dst, logvar_dst))")
        if _is_pair(out[0]):
            if not _is_pair(out[1]):
                raise TypeError("VGAE: the encoder returns (mu, logvar), or ((mu_src, logvar_src), (mu_dst, logvar_dst))")
            (mu_src, lv_src), (mu_dst, lv_dst) = out
            self.__mu__, self.__logvar__ = (mu_src, mu_dst), (lv_src, lv_dst)
        else:
            self.__mu__, self.__logvar__ = out
        return self.reparametrize(self.__mu__, self.__logvar__)

    def kl_loss(self, mu=None, logvar=None) -> torch.Tensor:
        """PyG's ``kl_loss``: ``-0.5 * mean(sum(1 + logvar - mu**2 - logvar.exp(), dim=1))`` with ``logvar`` clamped at
        ``MAX_LOGVAR`` -- without arguments the term of the last ``encode`` (from its own launch in training mode), with arguments
        a KL-only launch over them (tensors or pairs, the mean over all rows)."""
        if mu is None and logvar is None and self.__kl__ is not None:
            return self.__kl__
        mu = self.__mu__ if mu is None else mu
        logvar = self.__logvar__ if logvar is None else logvar
        if mu is None or logvar is None:
            raise ValueError("VGAE.kl_loss: no mu / logvar given and none kept by an encode()")
        if _is_pair(mu):
            n_total = int(mu[0].size(0)) + int(mu[1].size(0))
            return sum(F_.reparametrize_kl(m, lv, table=t, n_total=n_total, max_logvar=MAX_LOGVAR, sample=False)[1]
                       for t, (m, lv) in enumerate(zip(mu, logvar)))
        return F_.reparametrize_kl(mu, logvar, max_logvar=MAX_LOGVAR, sample=False)[1]


class ARGA(GAE):
    """PyG 1.4.2 ``ARGA(encoder, discriminator, decoder=None)``: ``GAE`` plus the adversarial regulariser, torch compositions over
    the user's ``discriminator`` (a module from ``z`` to one logit per row)."""

    def __init__(self, encoder, discriminator, decoder=None, **kwargs):
        super().__init__(encoder, decoder, **kwargs)
        self.discriminator = discriminator
        _reset(self.discriminator)

    def reset_parameters(self) -> None:
        super().reset_parameters()
        _reset(self.discriminator)

    def reg_loss(self, z: torch.Tensor) -> torch.Tensor:
        real = torch.sigmoid(self.discriminator(z))
        return -torch.log(real + EPS).mean()

    def discriminator_loss(self, z: torch.Tensor) -> torch.Tensor:
        real = torch.sigmoid(self.discriminator(torch.randn_like(z)))
        fake = torch.sigmoid(self.discriminator(z.detach()))
        return -torch.log(real + EPS).mean() - torch.log(1 - fake + EPS).mean()


class ARGVA(ARGA, VGAE):
    """PyG 1.4.2 ``ARGVA(encoder, discriminator, decoder=None)``: ``ARGA`` with ``VGAE``'s ``encode`` / ``reparametrize`` /
    ``kl_loss`` (and its ``seed`` / ``tick``)."""

    def __init__(self, encoder, discriminator, decoder=None, seed: int = 0, tick: Optional[torch.Tensor] = None):
        super().__init__(encoder, discriminator, decoder, seed=seed, tick=tick)
