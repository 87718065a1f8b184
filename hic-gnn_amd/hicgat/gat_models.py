"""The in-scope HiC-GNN models on the HIP path, with the reference's forward()/get_model() surface.

* ``GATNetSelectiveResidualsUpdated``       -- models.py:614-691 (flagship, 601 475 parameters).
* ``GATNetHeadsChanged3LayersLeakyReLUv2``  -- models.py:1010-1047 (411 651 parameters).
* ``Net``                                   -- models.py:14-55, the SAGEConv baseline (697 475).
* ``GATNetHeadsChangedLeakyReLU``           -- models.py:181-222, GATConv(512, 128, heads=2) (175 171).
* ``GATNetReduced``                         -- models.py:1414-1459, GATConv(512, 512, heads=2), the model
                                               evaluate.py:86 loads (806 403); inference only.

Four models that train with feature dropout (``_DropoutMLP``; ``ops.act_dropout``, dropout.hip):

* ``GATNet``                                    -- models.py:60-98, GATConv(512, 512), p = 0.3 at three
                                                   sites (436 355).
* ``GATNetHeadsChanged3LayersLeakyReLU``        -- models.py:971-1007, leaky_relu, p = 0.3 (428 291).
* ``GATNetHeadsChanged4LayerEmbedding512Dense`` -- models.py:1365-1411, p = 0.3 (438 339); the model
                                                   HiC-GNN_node2vec_conversion.py:134 trains.
* ``GATNetMoreReduced``                         -- models.py:1461-1494, p = 0.4.

Two more that also normalise with ``torch.nn.BatchNorm1d`` over the node rows (``_BatchNormMLP``;
``ops.bn_act_dropout``, batchnorm.hip), Dropout(0.4) at two sites:

* ``GATNetHeadsChanged4LayersLeakyReLU``       -- models.py:270-319 (437 251 parameters); the model
                                                  tune_hyperparams_embeddings.py:48 scores.
* ``GATNetHeadsChanged4LayersLeakyReLUHeads4`` -- models.py:834-883, GATConv(256, 256, heads=4) (569 859).

One that returns its attention weights and trains with an attention-entropy term through them
(``GATConv(..., return_attention_weights=True)``, gat_attn.hip):

* ``GATNetHeadsChanged3LayersEmbeddingDim256Entropy`` -- models.py:1112-1148, GATConv(256, 128, heads=2)
                                                         (107 651 parameters); 256 feature columns.

Six whose MLP tail normalises with ``torch.nn.LayerNorm`` like the flagship's, on the same row pass
(``_LayerNormTail``; ``ops.ln_act_res`` / ``ops.dual_ln_act_res`` / ``ops.act``, ln_act.hip), registered in
``LN_MODELS`` (``ALL_MODELS`` = ``MODELS`` then these); single-GPU ``hicgat.train`` only:

* ``GATNetHeadsChanged4LayersReLU_LayerNorm``      -- models.py:321-377, GATConv(256, 128, heads=2),
                                                      LayerNorm(128 / 64 / 32), relu; 256 feature columns.
* ``GATNetHeadsChanged4LayersLeakyReLU_LayerNorm`` -- models.py:776-832, the same with leaky_relu(0.01).
* ``GATNetHeadsChanged4LayersReLU_LayerNormEmbed512`` -- models.py:379-435, LayerNorm(256 / 128 / 64).
* ``GATNetSelectiveResiduals``                     -- models.py:528-612, three residual blocks.
* ``GATNetHeadsChanged4LayersReLU_LayerNormEmbed512WithResiduals`` -- models.py:437-526, ``conv1`` with
                                                      LayerNorm(512) and a residual of its own.
* ``GATNetSelectiveResidualsUpdatedLayerNorm``     -- models.py:693-773, gelu and a LayerNorm after each
                                                      residual add.

As in the reference, ``get_model`` never drops and ``forward`` / ``loss`` drop iff ``self.training``.
The masks are not torch's: they are a counter-based function of (seed, step, site, row, column)
(DESIGN.md "Feature dropout"), so a captured step replays them.  ``GATNetReduced`` still refuses to
train: lifting that is a one-line follow-up together with the two tests that pin the refusal.

Submodules are registered in the reference's order (so the same seed gives the same initial
weights and the same state_dict keys).  ``forward`` returns the N x N distance matrix like the
reference (``cdist`` on the GPU); ``get_model`` returns the N x 3 coordinates; ``loss`` is the
fused path used by the training loop (distance + MSE [+ Pearson] without materialising N x N).
"""
import torch
import torch.nn.functional as F
from torch.nn import BatchNorm1d, Dropout, LayerNorm, LeakyReLU, Linear

from . import ops
from .nn import GATConv, SAGEConv


def _lin(layer, x):
    """A torch.nn.Linear of the model, run on the MFMA GEMM kernels."""
    return ops.linear(x, layer.weight, layer.bias)


class _CoordsModel(torch.nn.Module):
    def flat_parameters(self):
        """Parameter order for ``FlatAdam``'s flat buffers (default: ``parameters()``)."""
        return list(self.parameters())

    def forward(self, x, edge_index):
        return ops.pairwise_dist(self.get_model(x, edge_index))

    def loss(self, x, edge_index, truth, kind="mse", tile_range=(0, -1), stats=None, alpha=1.0):
        """Fused ``criterion(model(x, ei), truth)``; returns ``(loss, stats, coords)``."""
        coords = self.get_model(x, edge_index)
        loss, stats = ops.fused_dist_loss(coords, truth, kind, tile_range, stats, alpha)
        return loss, stats, coords


class GATNetSelectiveResidualsUpdated(_CoordsModel):
    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 256)
        self.norm_a = LayerNorm(256)
        self.align_densea = Linear(512, 256)
        self.dense1 = Linear(256, 128)
        self.norm1 = LayerNorm(128)
        self.align_dense1 = Linear(256, 128)
        self.dense2 = Linear(128, 64)
        self.norm2 = LayerNorm(64)
        self.dense3 = Linear(64, 3)

    conv_act = "relu"   # the relu of models.py:637 runs in the GAT aggregation's epilogue

    def flat_parameters(self):
        """dense* / align_dense* weights and biases adjacent in the flat buffers, so each residual
        block's [W1; W2] and [b1; b2] are views (one GEMM / one column sum in the backward)."""
        return [self.conv.lin_l.weight, self.conv.att_l, self.conv.att_r, self.conv.bias,
                self.densea.weight, self.align_densea.weight, self.densea.bias, self.align_densea.bias,
                self.norm_a.weight, self.norm_a.bias,
                self.dense1.weight, self.align_dense1.weight, self.dense1.bias, self.align_dense1.bias,
                self.norm1.weight, self.norm1.bias,
                self.dense2.weight, self.dense2.bias, self.norm2.weight, self.norm2.bias,
                self.dense3.weight, self.dense3.bias]

    def post_act(self, x):
        """models.py:638-659 (after the relu): each residual block relu(norm(dense(x))) +
        align_dense(x) as one fused op (one GEMM over [W; W_align], one row pass);
        relu(norm2(dense2(.))); dense3.  On graphs of >= ops.FUSED_TAIL_MIN_M rows the whole forward
        is one kernel (ops.fused_tail, tail_fused.hip) with the same backward."""
        if ops.fused_tail_ok(self, x):
            return ops.fused_tail(self, x)
        x = ops.dual_ln_act_res(x, self.densea, self.align_densea, self.norm_a, "relu")
        x = ops.dual_ln_act_res(x, self.dense1, self.align_dense1, self.norm1, "relu")
        x = ops.ln_act_res(_lin(self.dense2, x), self.norm2, "relu")
        return _lin(self.dense3, x)

    def tail(self, x):
        """models.py:637-659 after the GATConv output."""
        return self.post_act(F.relu(x))

    def get_model(self, x, edge_index):
        return self.post_act(self.conv(x, edge_index, act=self.conv_act))


class GATNetHeadsChanged3LayersLeakyReLUv2(_CoordsModel):
    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 256)
        self.dense1 = Linear(256, 64)
        self.dense2 = Linear(64, 3)

    conv_act = None     # leaky_relu(0.01) stays a torch op on the GATConv output

    def tail(self, x):
        x = F.leaky_relu(x)
        x = F.leaky_relu(_lin(self.densea, x))
        x = F.leaky_relu(_lin(self.dense1, x))
        return _lin(self.dense2, x)

    post_act = tail

    def get_model(self, x, edge_index):
        return self.tail(self.conv(x, edge_index))


class GATNetHeadsChangedLeakyReLU(_CoordsModel):
    """models.py:181-222: GATConv(512, 128, heads=2) -> 256-128-64-32-3 with leaky_relu(0.01) between."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 128, heads=2, concat=True)
        self.densea = Linear(256, 128)
        self.dense1 = Linear(128, 64)
        self.dense2 = Linear(64, 32)
        self.dense3 = Linear(32, 3)
        self.leaky_relu = LeakyReLU()

    conv_act = None     # leaky_relu(0.01) stays a torch op on the GATConv output

    def tail(self, x):
        x = F.leaky_relu(x)
        x = F.leaky_relu(_lin(self.densea, x))
        x = F.leaky_relu(_lin(self.dense1, x))
        x = F.leaky_relu(_lin(self.dense2, x))
        return _lin(self.dense3, x)

    post_act = tail

    def get_model(self, x, edge_index):
        return self.tail(self.conv(x, edge_index))


class GATNetHeadsChanged3LayersEmbeddingDim256Entropy(_CoordsModel):
    """models.py:1112-1148: GATConv(256, 128, heads=2) called with ``return_attention_weights=True`` ->
    relu -> 256-128-64-3 with relu between (107 651 parameters); 256 feature columns.  ``forward`` returns
    ``(D, attn)`` like the reference (``attn``: see ``GATConv.forward``), ``get_model`` the coordinates.

    The reference carries ``self.alpha = 0.01`` for an attention-entropy term, but no script of it trains
    this model, so the objective is this project's: ``loss()`` returns

        fused_dist_loss(coords, truth, kind) + self.alpha * attention_entropy(alpha) / (N * H)

    -- the mean entropy per (row, head) of the attention distributions, weighted by ``self.alpha``
    (``ops.attention_entropy``).  Its gradient reaches the GATConv through the attention weights."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(256, 128, heads=2, concat=True)
        self.densea = Linear(256, 128)
        self.dense1 = Linear(128, 64)
        self.dense2 = Linear(64, 3)
        self.alpha = 0.01

    conv_act = "relu"   # the relu after the GATConv runs in the aggregation's epilogue

    def post_act(self, x):
        x = F.relu(_lin(self.densea, x))
        x = F.relu(_lin(self.dense1, x))
        return _lin(self.dense2, x)

    def tail(self, x):
        return self.post_act(F.relu(x))

    def coords_and_attention(self, x, edge_index):
        x, attn = self.conv(x, edge_index, act=self.conv_act, return_attention_weights=True)
        return self.post_act(x), attn

    def get_model(self, x, edge_index):
        return self.coords_and_attention(x, edge_index)[0]

    def forward(self, x, edge_index):
        coords, attn = self.coords_and_attention(x, edge_index)
        return ops.pairwise_dist(coords), attn

    def loss(self, x, edge_index, truth, kind="mse", tile_range=(0, -1), stats=None, alpha=1.0):
        coords, attn = self.coords_and_attention(x, edge_index)
        loss, stats = ops.fused_dist_loss(coords, truth, kind, tile_range, stats, alpha)
        w = attn.storage.value()
        loss = loss + (self.alpha / (x.shape[0] * w.shape[1])) * ops.attention_entropy(w)
        return loss, stats, coords


class GATNetReduced(_CoordsModel):
    """models.py:1414-1459: GATConv(512, 512, heads=2) -> relu -> 1024-256-64-3 with relu between.
    The reference's training ``forward`` applies Dropout(0.4) after the GATConv and after densea
    (``get_model`` does not); feature dropout is not implemented here, so in training mode ``forward``
    and ``loss`` refuse instead of training without it.  Eval mode and ``get_model`` run."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 512, heads=2, concat=True)
        self.densea = Linear(1024, 256)
        self.dense1 = Linear(256, 64)
        self.dense2 = Linear(64, 3)
        self.dropout = Dropout(p=0.4)

    conv_act = "relu"   # the relu after the GATConv runs in the aggregation's epilogue

    def post_act(self, x):
        x = F.relu(_lin(self.densea, x))
        x = F.relu(_lin(self.dense1, x))
        return _lin(self.dense2, x)

    def tail(self, x):
        return self.post_act(F.relu(x))

    def get_model(self, x, edge_index):
        return self.post_act(self.conv(x, edge_index, act=self.conv_act))

    def _no_training(self):
        if self.training:
            raise NotImplementedError("GATNetReduced trains with Dropout(0.4) in the reference (models.py:1432, "
                                      ":1438); feature dropout is not implemented, so the model runs in eval "
                                      "mode only (model.eval())")

    def forward(self, x, edge_index):
        self._no_training()
        return super().forward(x, edge_index)

    def loss(self, x, edge_index, truth, kind="mse", tile_range=(0, -1), stats=None, alpha=1.0):
        self._no_training()
        return super().loss(x, edge_index, truth, kind, tile_range, stats, alpha)


class _DropoutMLP(_CoordsModel):
    """The zoo's commonest shape: conv -> act -> k Linears with ``act`` between them, and in the
    training ``forward`` a Dropout after each of the first ``drop_sites`` activations (``get_model``
    never drops).  A subclass registers its submodules in the reference's order and names its
    Linears, in the order they run, in ``linears``.

    Eval mode is the plain path (relu in the aggregation's epilogue).  In training mode ``forward``
    and ``loss`` run the GATConv without an activation and each act -> dropout pair as one
    ``ops.act_dropout``; the masks come from the model's ``DropoutState`` (created on the input's
    device by the first training forward, seed = ``torch.initial_seed()``), which every training
    forward advances once, first."""

    act = "relu"        # or "leaky_relu" (slope 0.01)
    drop_sites = 2
    linears = ()

    def _act(self, x):
        return F.relu(x) if self.act == "relu" else F.leaky_relu(x)

    def get_model(self, x, edge_index):
        layers = [getattr(self, n) for n in self.linears]
        if self.act == "relu":
            x = self.conv(x, edge_index, act="relu")
        else:
            x = self._act(self.conv(x, edge_index))
        for lin in layers[:-1]:
            x = self._act(_lin(lin, x))
        return _lin(layers[-1], x)

    def dropout_state(self, device):
        """The model's ``DropoutState`` (made on first use; ``p`` from ``self.dropout``)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        st = getattr(self, "_dropout_state", None)
        if st is None or st.device != device:
            from .dropout import DropoutState
            st = self._dropout_state = DropoutState(device, p=self.dropout.p)
        return st

    def train_coords(self, x, edge_index):
        """The coordinates of one training forward (models.py ``forward`` before its cdist)."""
        st = self.dropout_state(x.device)
        st.advance()
        x = self.conv(x, edge_index, act=None)
        for k, name in enumerate(self.linears):
            x = ops.act_dropout(x, self.act, st.p, st, site=k) if k < self.drop_sites else self._act(x)
            x = _lin(getattr(self, name), x)
        return x

    def _coords(self, x, edge_index):
        return self.train_coords(x, edge_index) if self.training else self.get_model(x, edge_index)

    def forward(self, x, edge_index):
        return ops.pairwise_dist(self._coords(x, edge_index))

    def loss(self, x, edge_index, truth, kind="mse", tile_range=(0, -1), stats=None, alpha=1.0):
        coords = self._coords(x, edge_index)
        loss, stats = ops.fused_dist_loss(coords, truth, kind, tile_range, stats, alpha)
        return loss, stats, coords


class GATNet(_DropoutMLP):
    """models.py:60-98: GATConv(512, 512) -> 512-256-128-64-3, relu, Dropout(0.3) after the first three
    activations (436 355 parameters)."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 512)
        self.densea = Linear(512, 256)
        self.dense1 = Linear(256, 128)
        self.dense2 = Linear(128, 64)
        self.dense3 = Linear(64, 3)
        self.dropout = Dropout(p=0.3)

    drop_sites = 3
    linears = ("densea", "dense1", "dense2", "dense3")


class GATNetHeadsChanged3LayersLeakyReLU(_DropoutMLP):
    """models.py:971-1007: GATConv(512, 256, heads=2) -> 512-256-128-3, leaky_relu(0.01), Dropout(0.3)
    after the first two activations (428 291 parameters)."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 256)
        self.dense1 = Linear(256, 128)
        self.dense2 = Linear(128, 3)
        self.dropout = Dropout(p=0.3)

    act = "leaky_relu"
    linears = ("densea", "dense1", "dense2")


class GATNetHeadsChanged4LayerEmbedding512Dense(_DropoutMLP):
    """models.py:1365-1411, the model HiC-GNN_node2vec_conversion.py:134 trains: GATConv(512, 256,
    heads=2) -> 512-256-128-64-32-3, relu, Dropout(0.3) after the first two activations (438 339)."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 256)
        self.dense1 = Linear(256, 128)
        self.dense2 = Linear(128, 64)
        self.dense3 = Linear(64, 32)
        self.dense4 = Linear(32, 3)
        self.dropout = Dropout(p=0.3)

    linears = ("densea", "dense1", "dense2", "dense3", "dense4")


class GATNetMoreReduced(_DropoutMLP):
    """models.py:1461-1494: GATConv(512, 256, heads=2) -> 512-128-32-3, relu, Dropout(0.4) after the
    first two activations."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 128)
        self.dense1 = Linear(128, 32)
        self.dense2 = Linear(32, 3)
        self.dropout = Dropout(p=0.4)

    linears = ("densea", "dense1", "dense2")


class _BatchNormMLP(_DropoutMLP):
    """conv -> leaky_relu -> Dropout, then Linear -> BatchNorm1d -> leaky_relu (-> Dropout after the
    first) per hidden layer, then the last Linear (models.py:270-319, :834-883).  ``norms`` names the
    BatchNorm1d of each Linear but the last.  Dropout site 0 is the activation after the conv
    (``ops.act_dropout``), site 1 the one after ``bn_a``; every BatchNorm stage is one
    ``ops.bn_act_dropout`` (batchnorm.hip).

    Dropout runs only in a training ``forward`` / ``loss`` and never in ``get_model``.  BatchNorm
    follows ``self.training`` everywhere, ``get_model`` included: the reference's training scripts never
    call ``eval()``, so there ``get_model`` normalises by batch statistics and moves the running buffers
    (``num_batches_tracked`` counts it).  That is kept: call ``model.eval()`` for the running ones."""

    act = "leaky_relu"
    drop_sites = 2
    norms = ()

    def _mlp(self, x, st):
        """From the (dropped) activation of the conv's output on; ``st``: the DropoutState or None."""
        names = self.linears
        for k, (lin, bn) in enumerate(zip(names[:-1], self.norms)):
            drop = st is not None and k + 1 < self.drop_sites
            x = ops.bn_act_dropout(_lin(getattr(self, lin), x), getattr(self, bn), self.act,
                                   st if drop else None, k + 1 if drop else None)
        return _lin(getattr(self, names[-1]), x)

    def get_model(self, x, edge_index):
        return self._mlp(self._act(self.conv(x, edge_index)), None)

    def train_coords(self, x, edge_index):
        st = self.dropout_state(x.device)
        st.advance()
        x = ops.act_dropout(self.conv(x, edge_index, act=None), self.act, st.p, st, site=0)
        return self._mlp(x, st)


class GATNetHeadsChanged4LayersLeakyReLU(_BatchNormMLP):
    """models.py:270-319, the model tune_hyperparams_embeddings.py:48 loads: GATConv(512, 256, heads=2)
    -> 512-256-128-64-3 with BatchNorm1d after the first three Linears, leaky_relu(0.01), Dropout(0.4)
    after the conv's and bn_a's activations (437 251 parameters with the 896 of the BatchNorms)."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 256)
        self.bn_a = BatchNorm1d(256)
        self.dense1 = Linear(256, 128)
        self.bn1 = BatchNorm1d(128)
        self.dense2 = Linear(128, 64)
        self.bn2 = BatchNorm1d(64)
        self.dense3 = Linear(64, 3)
        self.dropout = Dropout(p=0.4)

    linears = ("densea", "dense1", "dense2", "dense3")
    norms = ("bn_a", "bn1", "bn2")


class GATNetHeadsChanged4LayersLeakyReLUHeads4(_BatchNormMLP):
    """models.py:834-883: GATConv(256, 256, heads=4) -> 1024-256-128-64-3, otherwise as
    ``GATNetHeadsChanged4LayersLeakyReLU`` (569 859 parameters); 256 feature columns."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(256, 256, heads=4, concat=True)
        self.densea = Linear(1024, 256)
        self.bn_a = BatchNorm1d(256)
        self.dense1 = Linear(256, 128)
        self.bn1 = BatchNorm1d(128)
        self.dense2 = Linear(128, 64)
        self.bn2 = BatchNorm1d(64)
        self.dense3 = Linear(64, 3)
        self.dropout = Dropout(p=0.4)

    linears = ("densea", "dense1", "dense2", "dense3")
    norms = ("bn_a", "bn1", "bn2")


class Net(_CoordsModel):
    """models.py:14-55: SAGEConv(512, 512) -> relu -> 512-256-128-64-3 with relu between."""

    def __init__(self):
        super().__init__()
        self.conv = SAGEConv(512, 512)
        self.densea = Linear(512, 256)
        self.dense1 = Linear(256, 128)
        self.dense2 = Linear(128, 64)
        self.dense3 = Linear(64, 3)

    def get_model(self, x, edge_index):
        x = F.relu(self.conv(x, edge_index))
        x = F.relu(_lin(self.densea, x))
        x = F.relu(_lin(self.dense1, x))
        x = F.relu(_lin(self.dense2, x))
        return _lin(self.dense3, x)


class _LayerNormTail(_CoordsModel):
    """The zoo's other LayerNorm tails: conv -> act, then stages ``(dense, norm, align, norm_residual)``
    (``stages``: attribute names, ``None`` where a stage has no residual Linear / second norm), each one
    ``norm_residual(act(norm(dense(x))) + align(x))`` as one GEMM (two Linears: over [W; W_align]) and one
    row pass (``ops.ln_act_res`` / ``ops.dual_ln_act_res``, ln_act.hip), then ``dense3``.  The reference's
    ``forward`` and ``get_model`` run the same layers, so training and eval share one path."""

    act = "relu"        # "relu", "leaky_relu" (slope 0.01) or "gelu", after the conv and after every norm
    stages = ()
    fused_tail = False  # not the flagship's tail: no one-kernel form, no weight pack in the step's first launch

    def flat_parameters(self):
        """``parameters()`` with each residual pair's weights, then its biases, adjacent (the dual-Linear
        backward's [dW; dW_align] and [db; db_align] are then one GEMM into FlatAdam's buffer)."""
        out, seen = [], set()
        pair = {id(getattr(self, d).weight): (getattr(self, d), getattr(self, a)) for d, _, a, _ in self.stages if a}
        for p in self.parameters():
            if id(p) in seen:
                continue
            group = [p]
            if id(p) in pair:
                lin, align = pair[id(p)]
                group = [lin.weight, align.weight, lin.bias, align.bias]
            out += group
            seen.update(id(q) for q in group)
        return out

    def conv_out(self, x, edge_index):
        """act(conv(x)): relu in the aggregation's epilogue, leaky_relu / gelu as one elementwise pass."""
        if self.act == "relu":
            return self.conv(x, edge_index, act="relu")
        return ops.act(self.conv(x, edge_index), self.act)

    def post_act(self, x):
        for dense, norm, align, norm_res in self.stages:
            n2 = getattr(self, norm_res) if norm_res else None
            if align:
                x = ops.dual_ln_act_res(x, getattr(self, dense), getattr(self, align), getattr(self, norm), self.act, n2)
            else:
                x = ops.ln_act_res(_lin(getattr(self, dense), x), getattr(self, norm), self.act, norm2=n2)
        return _lin(self.dense3, x)

    def get_model(self, x, edge_index):
        return self.post_act(self.conv_out(x, edge_index))


class GATNetHeadsChanged4LayersReLU_LayerNorm(_LayerNormTail):
    """models.py:321-377: GATConv(256, 128, heads=2) -> relu -> 256-128-64-32-3 with LayerNorm -> relu after
    the first three Linears (110 083 parameters); 256 feature columns."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(256, 128, heads=2, concat=True)
        self.densea = Linear(256, 128)
        self.norm_a = LayerNorm(128)
        self.dense1 = Linear(128, 64)
        self.norm1 = LayerNorm(64)
        self.dense2 = Linear(64, 32)
        self.norm2 = LayerNorm(32)
        self.dense3 = Linear(32, 3)

    stages = (("densea", "norm_a", None, None), ("dense1", "norm1", None, None), ("dense2", "norm2", None, None))


class GATNetHeadsChanged4LayersLeakyReLU_LayerNorm(GATNetHeadsChanged4LayersReLU_LayerNorm):
    """models.py:776-832: the same layers with F.leaky_relu (slope 0.01) in place of every relu."""

    act = "leaky_relu"


class GATNetHeadsChanged4LayersReLU_LayerNormEmbed512(_LayerNormTail):
    """models.py:379-435: GATConv(512, 256, heads=2) -> relu -> 512-256-128-64-3 with LayerNorm -> relu after
    the first three Linears."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 256)
        self.norm_a = LayerNorm(256)
        self.dense1 = Linear(256, 128)
        self.norm1 = LayerNorm(128)
        self.dense2 = Linear(128, 64)
        self.norm2 = LayerNorm(64)
        self.dense3 = Linear(64, 3)

    stages = (("densea", "norm_a", None, None), ("dense1", "norm1", None, None), ("dense2", "norm2", None, None))


class GATNetHeadsChanged4LayersReLU_LayerNormEmbed512WithResiduals(_LayerNormTail):
    """models.py:437-526: the conv is registered as ``conv1`` and is itself a residual block,
    relu(LayerNorm(512)(conv1(x))) + align1(x) on the raw features; then three residual blocks
    relu(norm(dense(x))) + align(x) and dense3."""

    def __init__(self):
        super().__init__()
        self.conv1 = GATConv(512, 256, heads=2, concat=True)
        self.norm1 = LayerNorm(512)
        self.densea = Linear(512, 256)
        self.norm_a = LayerNorm(256)
        self.dense1 = Linear(256, 128)
        self.norm1_2 = LayerNorm(128)
        self.dense2 = Linear(128, 64)
        self.norm2 = LayerNorm(64)
        self.dense3 = Linear(64, 3)
        self.align1 = Linear(512, 512)
        self.align_a = Linear(512, 256)
        self.align1_2 = Linear(256, 128)
        self.align2 = Linear(128, 64)

    stages = (("densea", "norm_a", "align_a", None), ("dense1", "norm1_2", "align1_2", None),
              ("dense2", "norm2", "align2", None))

    def conv_out(self, x, edge_index):
        return ops.ln_act_res(self.conv1(x, edge_index), self.norm1, "relu", res=_lin(self.align1, x))


class GATNetSelectiveResiduals(_LayerNormTail):
    """models.py:528-612: the flagship's predecessor -- GATConv(512, 256, heads=2) -> relu, then THREE
    residual blocks relu(norm(dense(x))) + align_dense(x) (the flagship dropped the third), dense3."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 256)
        self.norm_a = LayerNorm(256)
        self.align_densea = Linear(512, 256)
        self.dense1 = Linear(256, 128)
        self.norm1 = LayerNorm(128)
        self.align_dense1 = Linear(256, 128)
        self.dense2 = Linear(128, 64)
        self.norm2 = LayerNorm(64)
        self.align_dense2 = Linear(128, 64)
        self.dense3 = Linear(64, 3)

    stages = (("densea", "norm_a", "align_densea", None), ("dense1", "norm1", "align_dense1", None),
              ("dense2", "norm2", "align_dense2", None))


class GATNetSelectiveResidualsUpdatedLayerNorm(_LayerNormTail):
    """models.py:693-773: the flagship's layers with F.gelu for every relu and a second LayerNorm after each
    residual add: norm_residual(gelu(norm(dense(x))) + align_dense(x)) twice, gelu(norm2(dense2(x))),
    dense3."""

    def __init__(self):
        super().__init__()
        self.conv = GATConv(512, 256, heads=2, concat=True)
        self.densea = Linear(512, 256)
        self.norm_a = LayerNorm(256)
        self.align_densea = Linear(512, 256)
        self.norm_residual_a = LayerNorm(256)
        self.dense1 = Linear(256, 128)
        self.norm1 = LayerNorm(128)
        self.align_dense1 = Linear(256, 128)
        self.norm_residual_1 = LayerNorm(128)
        self.dense2 = Linear(128, 64)
        self.norm2 = LayerNorm(64)
        self.dense3 = Linear(64, 3)

    act = "gelu"
    stages = (("densea", "norm_a", "align_densea", "norm_residual_a"),
              ("dense1", "norm1", "align_dense1", "norm_residual_1"), ("dense2", "norm2", None, None))


MODELS = {
    "GATNetSelectiveResidualsUpdated": GATNetSelectiveResidualsUpdated,
    "GATNetHeadsChanged3LayersLeakyReLUv2": GATNetHeadsChanged3LayersLeakyReLUv2,
    "Net": Net,
    "GATNetHeadsChangedLeakyReLU": GATNetHeadsChangedLeakyReLU,
    "GATNetReduced": GATNetReduced,
    "GATNet": GATNet,
    "GATNetHeadsChanged3LayersLeakyReLU": GATNetHeadsChanged3LayersLeakyReLU,
    "GATNetHeadsChanged4LayerEmbedding512Dense": GATNetHeadsChanged4LayerEmbedding512Dense,
    "GATNetMoreReduced": GATNetMoreReduced,
    "GATNetHeadsChanged4LayersLeakyReLU": GATNetHeadsChanged4LayersLeakyReLU,
    "GATNetHeadsChanged4LayersLeakyReLUHeads4": GATNetHeadsChanged4LayersLeakyReLUHeads4,
    "GATNetHeadsChanged3LayersEmbeddingDim256Entropy": GATNetHeadsChanged3LayersEmbeddingDim256Entropy,
}

# the LayerNorm tails on the general row pass (ln_act.hip); single-GPU hicgat.train only
LN_MODELS = {
    "GATNetHeadsChanged4LayersReLU_LayerNorm": GATNetHeadsChanged4LayersReLU_LayerNorm,
    "GATNetHeadsChanged4LayersLeakyReLU_LayerNorm": GATNetHeadsChanged4LayersLeakyReLU_LayerNorm,
    "GATNetHeadsChanged4LayersReLU_LayerNormEmbed512": GATNetHeadsChanged4LayersReLU_LayerNormEmbed512,
    "GATNetSelectiveResiduals": GATNetSelectiveResiduals,
    "GATNetHeadsChanged4LayersReLU_LayerNormEmbed512WithResiduals":
        GATNetHeadsChanged4LayersReLU_LayerNormEmbed512WithResiduals,
    "GATNetSelectiveResidualsUpdatedLayerNorm": GATNetSelectiveResidualsUpdatedLayerNorm,
}
ALL_MODELS = {**MODELS, **LN_MODELS}


def model_class(name):
    """The class behind a ``--model`` name: ``MODELS`` first, then ``LN_MODELS``."""
    return MODELS[name] if name in MODELS else LN_MODELS[name]
