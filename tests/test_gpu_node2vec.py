"""``npi.Node2Vec`` on the GPU: the loss and its gradient against PyG 1.4.2's ``Node2Vec.loss`` expression evaluated by torch in
float64 on the same walks and negatives (taken from the numpy restatement ``tests/_walk_ref.py``), reproducibility, and training.

The bar is the project's for this path (``tests/test_gpu_link.py``): ``_util.rel_max <= _util.GRAD_REL``.  The embedding is drawn
from U(-0.25, 0.25), so a logit over D <= 64 columns stays within 64 * 0.25^2 = 4 (asserted), beyond which ``1 - sigmoid(x)`` loses
digits in float32 -- PyG's formula, not the kernel."""
import numpy as np
import pytest
import torch

import npi_gnn_amd as npi
from npi_gnn_amd import graph as NG
import _walk_ref as ref
from _util import GRAD_REL, rel_max
from test_walk_cpu import branchy_graph

pytestmark = pytest.mark.gpu

EPS = 1e-15
N, L, C, WPN = 300, 8, 4, 2


def _undirected():
    ei, n = branchy_graph()
    assert n == N
    return np.concatenate([ei, ei[::-1]], axis=1)


def _pyg_loss64(weight, walks, neg_sample, c):
    """PyG 1.4.2 ``Node2Vec.loss`` from ``rw`` on: the windows, ``start`` / ``rest``, the two means; float64"""
    rw = torch.from_numpy(walks)
    walk = torch.cat([rw[:, j:j + c] for j in range(1 + L + 1 - c)], dim=0)
    start, rest = walk[:, 0], walk[:, 1:].contiguous()
    emb = weight.double().clone().requires_grad_(True)
    D = emb.size(1)
    h_start = emb[start].view(walk.size(0), 1, D)
    h_rest = emb[rest.view(-1)].view(walk.size(0), rest.size(1), D)
    out_pos = (h_start * h_rest).sum(dim=-1).view(-1)
    pos_loss = -torch.log(torch.sigmoid(out_pos) + EPS).mean()
    h_neg_rest = emb[neg_sample]
    out_neg = (h_start * h_neg_rest).sum(dim=-1).view(-1)
    neg_loss = -torch.log(1 - torch.sigmoid(out_neg) + EPS).mean()
    loss = pos_loss + neg_loss
    loss.backward()
    assert float(torch.cat([out_pos, out_neg]).detach().abs().max()) <= 4.0
    return loss.detach(), emb.grad


def _model(dev, D, **kw):
    model = npi.Node2Vec(N, D, walk_length=L, context_size=C, walks_per_node=WPN, **kw).to(dev)
    with torch.no_grad():
        model.embedding.weight.copy_((torch.rand(N, D, generator=torch.Generator().manual_seed(D)) - 0.5) * 0.5)
    return model


def test_state_dict_layout(dev):
    model = _model(dev, 64)
    sd = model.state_dict()
    assert list(sd) == ["embedding.weight"] and tuple(sd["embedding.weight"].shape) == (N, 64) and sd["embedding.weight"].is_cuda
    z = model(torch.tensor([5, 7, 5], device=dev))
    assert torch.equal(z, model.embedding.weight[[5, 7, 5]])


@pytest.mark.parametrize("pq", [(1, 1), (0.5, 2)])
@pytest.mark.parametrize("D", [64, 30])
def test_loss_and_gradient_against_pygs_expression_in_float64(dev, D, pq):
    ei = _undirected()
    model = _model(dev, D, p=pq[0], q=pq[1], seed=2)
    model.draw = 3
    subset = np.random.default_rng(1).permutation(N)[:250]
    key = ref.epoch_seed(2, 3)
    walks, exhausted = ref.walks(key, ei, N, np.tile(subset, WPN), L, thr=ref.thresholds(*pq))    # subset.repeat(walks_per_node)
    assert exhausted == 0
    pairs, n_pos = ref.pairs(key, walks, C, C - 1, N)
    R = n_pos // (C - 1)
    want_loss, want_grad = _pyg_loss64(model.embedding.weight.detach().cpu(), walks, torch.from_numpy(pairs[1, n_pos:]).view(R, C - 1), C)
    NG.check_pending()
    loss = model.loss(_t(ei, dev), _t(subset, dev))
    assert loss.shape == () and loss.dtype == torch.float32 and model.draw == 4
    loss.backward()
    NG.check_pending()                                                             # every id in range, no step out of tries
    grad = model.embedding.weight.grad
    errs = rel_max(loss, want_loss), rel_max(grad, want_grad)
    print("rel_max of loss, gradient:", errs)
    assert errs[0] <= GRAD_REL and errs[1] <= GRAD_REL, errs
    # the sample the loss was taken over is the restatement's
    model.draw = 3
    w, p, npos = model.sample(_t(ei, dev), _t(subset, dev))
    assert npos == n_pos and torch.equal(w.cpu(), torch.from_numpy(walks)) and torch.equal(p.cpu(), torch.from_numpy(pairs))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_same_draw_same_bits(dev):
    ei = _t(_undirected(), dev)
    model = _model(dev, 64, p=0.5, q=2)
    out = []
    for _ in range(2):
        model.draw = 7
        model.zero_grad(set_to_none=True)
        loss = model.loss(ei)                                                       # subset=None: every node
        loss.backward()
        out.append((loss.detach().clone(), model.embedding.weight.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert len(model._walkers) == 1                                                 # one sort for the edge list that stays
    loss = model.loss(ei)                                                           # draw 8: other walks, another value
    assert model.draw == 9 and not torch.equal(loss.detach(), out[0][0])
    NG.check_pending()


def test_training_lowers_the_loss(dev):
    """two cliques of 10 nodes joined by nothing: twenty Adam steps; the loss of the last step lies below that of the first"""
    a = np.array([(i, j) for i in range(10) for j in range(10) if i != j]).T
    ei = _t(np.concatenate([a, a + 10], axis=1), dev)
    torch.manual_seed(0)
    model = npi.Node2Vec(20, 16, walk_length=8, context_size=4, walks_per_node=4).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = model.loss(ei)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("loss, steps 0 and 19:", losses[0], losses[-1])
    assert model.draw == 20 and losses[-1] < losses[0], losses
    NG.check_pending()
