"""fp64-capable torch restatement of the bipartite ``(x_src, x_dst)`` / ``size=`` forms of PyG 1.4.2 ``SAGEConv`` and ``GATConv``
(``MessagePassing.propagate`` with ``flow='source_to_target'``: ``edge_index[0]`` indexes the source table, ``edge_index[1]`` the
target rows; no self loop is added or removed).  Differentiable; pinned to ``oracle/ref_conv.py`` by ``tests/test_bipartite_cpu.py``.
Columns with an id out of range -- the ``(-1, -1)`` padding included -- are dropped first, as the graph build drops them."""
import torch


def _valid(edge_index, n_src, n_dst):
    s, d = edge_index[0], edge_index[1]
    return (s >= 0) & (s < n_src) & (d >= 0) & (d < n_dst)


def sage_bipartite(x_src, edge_index, weight, bias=None, n_dst=None, res_n_id=None, concat=False, edge_weight=None,
                   normalize=False, relu=False):
    n_src = x_src.size(0)
    n_dst = n_src if n_dst is None else int(n_dst)
    keep = _valid(edge_index, n_src, n_dst)
    s, d = edge_index[0][keep], edge_index[1][keep]
    msg = x_src.index_select(0, s)
    if edge_weight is not None:
        msg = edge_weight.view(-1)[keep].view(-1, 1) * msg
    agg = torch.zeros((n_dst, x_src.size(1)), dtype=x_src.dtype).index_add_(0, d, msg)
    cnt = torch.zeros(n_dst, dtype=x_src.dtype).index_add_(0, d, torch.ones_like(d, dtype=x_src.dtype))
    agg = agg / cnt.clamp(min=1).view(-1, 1)
    if concat:
        root = x_src.index_select(0, res_n_id)
        agg = torch.cat([root, agg], dim=-1)
    out = agg @ weight
    if bias is not None:
        out = out + bias
    if relu:
        out = torch.relu(out)
    if normalize:
        out = torch.nn.functional.normalize(out, p=2.0, dim=-1)
    return out


def gat_bipartite(x_src, x_dst, edge_index, weight, att, bias=None, n_dst=None, heads=1, concat=True, negative_slope=0.2, relu=False):
    n_src = x_src.size(0)
    n_dst = (x_dst.size(0) if x_dst is not None else n_src) if n_dst is None else int(n_dst)
    H = int(heads)
    C = weight.size(1) // H
    keep = _valid(edge_index, n_src, n_dst)
    s, d = edge_index[0][keep], edge_index[1][keep]
    h_src = (x_src @ weight).view(n_src, H, C)
    a = att.view(1, H, 2 * C)
    e = (h_src.index_select(0, s) * a[:, :, C:]).sum(-1)                          # [E, H]
    if x_dst is not None:
        h_dst = (x_dst @ weight).view(n_dst, H, C)
        e = e + (h_dst.index_select(0, d) * a[:, :, :C]).sum(-1)
    e = torch.nn.functional.leaky_relu(e, negative_slope)
    mx = torch.full((n_dst, H), -1e38, dtype=e.dtype).scatter_reduce(0, d.view(-1, 1).expand_as(e), e, reduce="amax", include_self=True)
    ex = (e - mx.index_select(0, d)).exp()
    den = torch.zeros((n_dst, H), dtype=e.dtype).index_add_(0, d, ex)
    alpha = ex / (den.index_select(0, d) + 1e-16)
    out = torch.zeros((n_dst, H, C), dtype=e.dtype).index_add_(0, d, alpha.unsqueeze(-1) * h_src.index_select(0, s))
    out = out.reshape(n_dst, H * C) if concat else out.mean(dim=1)
    if bias is not None:
        out = out + bias
    return torch.relu(out) if relu else out
