"""``GATConv``: drop-in for PyG 1.7.2 ``torch_geometric.nn.GATConv`` on the HIP kernels.

Same constructor arguments, parameter names and state_dict keys as the version the reference
instantiates (``models.py:619``: ``GATConv(512, 256, heads=2, concat=True)``):
``lin_l.weight`` [H*C, F] (no bias; ``lin_r`` is the same module, so ``lin_r.weight`` aliases it
in the state_dict exactly like PyG), ``att_l`` / ``att_r`` [1, H, C], ``bias`` [H*C].  The RNG
draws of the initialisation follow PyG 1.7.2 (``torch.nn.Linear``'s own init, then glorot on
lin_l, glorot on lin_r (the same tensor), glorot on att_l, att_r, zeros on bias), so
``torch.manual_seed(s)`` gives the reference's initial weights bit for bit.

``dropout`` = p in [0, 1) is PyG's dropout on the attention coefficients: in training mode every
alpha_ij is multiplied by a keep factor in {0, 1 / (1 - p)} per head inside the aggregation kernels
(DESIGN.md "Attention dropout").  It adds no parameter, buffer or RNG draw.  Out of scope (refused):
``concat=False``, ``add_self_loops=False``, bipartite inputs.
"""
import math

import torch
from torch.nn import Linear, Parameter

from . import ops
from .dropout import check_p


def _glorot(t):
    stdv = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-stdv, stdv)


class GATConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2,
                 dropout=0.0, add_self_loops=True, bias=True, **kwargs):
        super().__init__()
        if not isinstance(in_channels, int):
            raise NotImplementedError("bipartite (tuple) in_channels is out of scope")
        if not concat:
            raise NotImplementedError("concat=False (head mean) is out of scope")
        dropout = check_p(dropout)
        if not add_self_loops:
            raise NotImplementedError("add_self_loops=False is out of scope")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope = concat, negative_slope
        self.dropout, self.add_self_loops = dropout, add_self_loops
        self.lin_l = Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = self.lin_l
        self.att_l = Parameter(torch.Tensor(1, heads, out_channels))
        self.att_r = Parameter(torch.Tensor(1, heads, out_channels))
        if bias:
            self.bias = Parameter(torch.Tensor(heads * out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.lin_l.weight)
        _glorot(self.lin_r.weight)
        _glorot(self.att_l)
        _glorot(self.att_r)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def dropout_state(self, device):
        """The conv's own ``DropoutState`` (made on first use on ``device``, seed ``torch.initial_seed()``:
        read, not drawn)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        st = getattr(self, "_dropout_state", None)
        if st is None or st.device != device:
            from .dropout import DropoutState
            st = self._dropout_state = DropoutState(device)
        return st

    def forward(self, x, edge_index, act=None, return_attention_weights=None, dropout_state=None, site=0):
        """``edge_index`` is a ``hicgat.graph.Adj`` (the reference passes a SparseTensor).
        In training mode with ``self.dropout`` > 0 (read here, so it may be set on the module as in PyG)
        the attention coefficients are dropped; the returned attention weights are the undropped ones,
        as PyG's.  The mask comes from ``dropout_state`` (a ``DropoutState`` the caller advances once per
        training forward, shared with its other dropout sites) and ``site``; without one the conv owns
        a state and advances it itself, first in the forward.
        ``act="relu"`` (not in PyG) returns relu(forward(x)) with the relu fused into the kernel.
        ``return_attention_weights=True`` returns ``(out, attn)`` as PyG does for a SparseTensor input
        (``edge_index.set_value(alpha, layout='coo')``): ``attn`` is an ``Adj`` over the self-looped CSR
        whose ``storage.rowptr()`` / ``col()`` are int64 and whose ``storage.value()`` is alpha [nnz, H],
        attached to autograd (a loss may depend on it)."""
        drop = {}
        p = check_p(self.dropout)
        if self.training and p > 0.0:
            if dropout_state is None:
                dropout_state = self.dropout_state(x.device)
                dropout_state.advance()
            drop = dict(dropout=p, training=True, state=dropout_state, site=site)
        if not return_attention_weights:
            return ops.gat_conv(x, self.lin_l.weight, self.att_l, self.att_r, self.bias, edge_index,
                                self.negative_slope, act, **drop)
        out, alpha = ops.gat_conv(x, self.lin_l.weight, self.att_l, self.att_r, self.bias, edge_index,
                                  self.negative_slope, act, return_attention_weights=True, **drop)
        return out, edge_index.with_self_loops(alpha)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"


class SAGEConv(torch.nn.Module):
    """Drop-in for the reference's own ``layers.SAGEConv`` (layers.py:12-79).

    Same parameters and state_dict keys (``lin_l.weight``, ``lin_l.bias``, ``lin_r.weight``) and
    the same init (torch.nn.Linear's, in construction order: the reference never calls its
    ``reset_parameters``, layers.py:33).  ``forward`` keeps the degree normalisation
    ``diag(1/colsum) @ adj`` and the ``x.long()`` truncation of the root branch (layers.py:64)."""

    def __init__(self, in_channels, out_channels, normalize=False, root_weight=True, bias=True, **kwargs):
        super().__init__()
        if not isinstance(in_channels, int):
            raise NotImplementedError("bipartite (tuple) in_channels is out of scope")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.normalize, self.root_weight = normalize, root_weight
        self.lin_l = Linear(in_channels, out_channels, bias=bias)
        if root_weight:
            self.lin_r = Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        if self.root_weight:
            self.lin_r.reset_parameters()

    def forward(self, x, edge_index):
        out = ops.sage_conv(x, self.lin_l.weight, self.lin_l.bias,
                            self.lin_r.weight if self.root_weight else None, edge_index)
        if self.normalize:
            out = torch.nn.functional.normalize(out, p=2.0, dim=-1)
        return out

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"
