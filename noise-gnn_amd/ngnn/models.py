"""Drop-in model wrappers: ``SAGE``, ``SAGEH``, ``SAGEPL``, ``SimpleGCN`` and the ``NGNN`` factory.

Mirror the reference classes one to one:

* ``SAGE``      src/models/layers/sage.py:6-79
* ``SAGEH``     src/models/layers/sageH.py:6-35
* ``SAGEPL``    src/models/layers/sagePL.py:6-94
* ``SimpleGCN`` src/models/layers/convolution.py:7-53
* ``NGNN``      src/models/model.py:10-69 (module string -> network, Adam optimiser)

Differences are internal only: ``forward`` builds the validated CSR
:class:`~ngnn.block.Block` once per call and hands it to every layer (the
reference's PyG convs re-scan ``edge_index`` per layer), and ``inference``
keeps each layer's activations on the device (see its docstring).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused, infer
from .block import get_block
from .infer import last_inference_plan  # noqa: F401  (per layer: "rowtile" / "narrow" / "loop")
from .loader import IndexedRows
from .nn import GCNConv, SAGEConv
from .ops import add_node_noise, batch_norm_act, batch_norm_act_supported


def _refuse_sync_free(edge_index):
    """A NeighborLoader(sync_free=True) batch holds capacity-sized buffers
    whose real extent only the device knows (ABI 19): refused before anything
    reads them (ngnn.block.get_block checks again for direct conv calls)."""
    if getattr(edge_index, "_ngnn_counts", None) is not None:
        raise ValueError("a sync_free NeighborLoader batch feeds GraphedTrainStep only; "
                         "use NeighborLoader(sync_free=False) for eager training")


def _dropout_seed(model, x, block, training=None):
    """(host seed, device seed word) of a fused stack's hash dropout;
    training: what decides the dropout (default: model.training)."""
    seed, seed_dev = 0, None
    if (model.training if training is None else training) and model.dropout > 0:
        if torch.cuda.is_current_stream_capturing():
            # HIP-graph capture: a device seed, fresh at every replay -- the
            # slot's (advanced by each slot load), else drawn by torch's
            # graph-safe generator inside the graph.  The host part is the
            # model's graph salt (0 unless set: two models captured over one
            # slot -- GraphedCoTeachingStep -- draw independent masks)
            seed = int(getattr(model, "_ngnn_graph_salt", 0))
            seed_dev = block.seed_dev
            if seed_dev is None:
                seed_dev = torch.randint(0, 2**62, (1,), device=x.device)
        else:
            seed = int(torch.randint(0, 2**62, (1,)).item())  # torch's (CPU) RNG stream
    return seed, seed_dev


class SAGE(nn.Module):
    def __init__(self, in_size, hidden_size, out_size, num_layers, dropout=0.5, use_bn=False,
                 aggr: str = "mean"):
        super().__init__()
        self.num_layers = num_layers
        self.dropout = dropout
        self.convs = nn.ModuleList()
        self.convs.append(SAGEConv(in_size, hidden_size, aggr=aggr))
        for _ in range(num_layers - 2):
            self.convs.append(SAGEConv(hidden_size, hidden_size, aggr=aggr))
        self.convs.append(SAGEConv(hidden_size, out_size, aggr=aggr))
        self.use_bn = use_bn
        if self.use_bn:
            self.bn1 = nn.BatchNorm1d(in_size)
            self.bn2 = nn.BatchNorm1d(hidden_size)

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x, edge_index):
        _refuse_sync_free(edge_index)
        if isinstance(x, IndexedRows):  # eager: gather the rows (graph replays fuse it)
            x = x.materialize()
        block = get_block(edge_index, x.size(0))
        if fused.sage_stack_supported(self, x):
            # one autograd node for the stack: fused layer kernels forward,
            # receptive-field-bounded backward (ngnn/fused.py)
            return fused.sage_stack(self, x, block, *_dropout_seed(self, x, block))
        if self.use_bn:
            x = batch_norm_act(x, self.bn1)
        seeds = None
        for i, conv in enumerate(self.convs):
            x = conv(x, block)
            if i != self.num_layers - 1:
                if self.use_bn:
                    # ReLU, BatchNorm and dropout in one op (ngnn.ops.batch_norm_act:
                    # HIP kernels when eager fp32, torch's ops otherwise); one
                    # hash-dropout seed per call, stepped per layer as the fused
                    # stack's, and drawn only when the kernels will use it
                    if seeds is None:
                        seeds = _dropout_seed(self, x, block) \
                            if batch_norm_act_supported(x, self.bn2, self.training) else (0, None)
                    x = batch_norm_act(x, self.bn2, relu=True, p=self.dropout, seed=seeds[0] + 7919 * i,
                                       seed_dev=seeds[1])
                else:
                    x = x.relu()
                    x = F.dropout(x, p=self.dropout, training=self.training)
        return x

    @torch.no_grad()
    def inference(self, x_all, subgraph_loader, device):
        """Layer-wise inference, sage.py:42-58 semantics.

        Per layer i and per loader batch: ``convs[i](x_all[n_id], edge_index)[:batch_size]``,
        relu except after the last layer, rows concatenated in loader order.
        ``x_all`` may live on the host (as in the reference) or on the device;
        the result is returned where ``x_all`` was given.  Between layers the
        activations stay on the device (the reference round-trips every batch
        through the host, sage.py:50,56).

        With an in-order ``ngnn.loader.NeighborLoader`` over every node the
        same rows are computed without building a block (ngnn.infer: the seed
        rows' hop-0 draws straight from the graph CSR; ``last_inference_plan``
        names each layer's path).
        """
        return _inference(self.convs, self.num_layers, x_all, subgraph_loader, device)


class SimpleGCN(nn.Module):
    def __init__(self, in_size, hidden_size, out_size, num_layers, dropout=0.5, use_bn=False,
                 normalize=False):
        super().__init__()
        self.num_layers = num_layers
        self.dropout = dropout
        # normalize=True: every layer is the symmetric-normalised GCNConv (not
        # the reference's choice, convolution.py:19-23; the per-conv path)
        self.normalize = bool(normalize)
        self.convs = nn.ModuleList()
        self.convs.append(GCNConv(in_size, hidden_size, normalize=normalize))
        for _ in range(num_layers - 2):
            self.convs.append(GCNConv(hidden_size, hidden_size, normalize=normalize))
        self.convs.append(GCNConv(hidden_size, out_size, normalize=normalize))

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x, edge_index):
        _refuse_sync_free(edge_index)
        if isinstance(x, IndexedRows):  # eager: gather the rows (graph replays fuse it)
            x = x.materialize()
        block = get_block(edge_index, x.size(0))
        if fused.gcn_stack_supported(self, x):
            # one autograd node for the stack (ngnn/fused.py: SAGE layers with
            # W_r = 0, sum aggregation); dropout seed as SAGE.forward
            return fused.gcn_stack(self, x, block, *_dropout_seed(self, x, block))
        for i, conv in enumerate(self.convs):
            x = conv(x, block)
            if i != self.num_layers - 1:
                x = x.relu()
                x = F.dropout(x, p=self.dropout, training=self.training)
        return x

    @torch.no_grad()
    def inference(self, x_all, subgraph_loader, device):
        """convolution.py:37-53 semantics (same loop, and the same block-free
        plan, as SAGE.inference)."""
        return _inference(self.convs, self.num_layers, x_all, subgraph_loader, device)


def _tapped_composition(convs, x, block, dropout, training):
    """(logits, h) layer by layer on the per-conv path: relu and F.dropout as
    torch ops, h the last hidden activation before dropout."""
    h = None
    for i, conv in enumerate(convs):
        x = conv(x, block)
        if i != len(convs) - 1:
            h = x.relu()
            x = F.dropout(h, p=dropout, training=training)
    return x, h


class SAGEH(nn.Module):
    """The reference's ``SAGEH`` (src/models/layers/sageH.py:6-35, what
    ``module: 'sageH'`` selects): a GraphSAGE stack whose forward returns
    ``(logits, h_out)``, ``h_out`` the last hidden activation after ReLU and
    before dropout.  One autograd node with two outputs on the fused
    per-layer kernels (``fused.sage_stack_tap``); inputs outside its envelope
    (non-fp32) take the per-conv composition.

    ``act`` and ``bnl`` are the reference's unused members (sageH.py:14,21),
    kept so that its checkpoints load with ``strict=True``.  Dropout follows
    the ``training`` ARGUMENT of forward, not ``self.training``
    (sageH.py:27,34).  ``num_layers >= 2``: with one layer the reference's
    ``h_out`` is never assigned and its forward raises; here the constructor
    does.  No ``inference`` method, as the reference has none.
    """

    def __init__(self, in_size, hidden_size, out_size, num_layers, dropout=0.5, aggr: str = "mean"):
        super().__init__()
        if num_layers < 2:
            raise ValueError("SAGEH needs num_layers >= 2: the hidden state it returns is the last "
                             "hidden layer's (undefined in the reference for one layer)")
        self.num_layers = num_layers
        self.dropout = dropout
        self.act = nn.PReLU()
        self.convs = nn.ModuleList()
        self.convs.append(SAGEConv(in_size, hidden_size, aggr=aggr))
        for _ in range(num_layers - 2):
            self.convs.append(SAGEConv(hidden_size, hidden_size, aggr=aggr))
        self.convs.append(SAGEConv(hidden_size, out_size, aggr=aggr))
        self.bnl = nn.BatchNorm1d(128)

    def reset_parameters(self):
        for conv in self.convs:  # (the convs only, as the reference: sageH.py:23-25)
            conv.reset_parameters()

    def forward(self, x, edge_index, training=True):
        _refuse_sync_free(edge_index)
        if isinstance(x, IndexedRows):  # eager: gather the rows
            x = x.materialize()
        block = get_block(edge_index, x.size(0))
        if fused.sage_tap_supported(self, x):
            seed, seed_dev = _dropout_seed(self, x, block, training=training)
            return fused.sage_stack_tap(self, x, block, seed, seed_dev, training=training)
        return _tapped_composition(self.convs, x, block, self.dropout, training)


class SAGEPL(nn.Module):
    """The reference's ``SAGEPL`` (src/models/layers/sagePL.py:6-94, what
    ``module: 'sagePL'`` selects): a GraphSAGE stack with a learnable noise
    table ``noise [nbr_nodes, in_size]``.  Each call runs a pure pass on ``x``
    and a noisy pass on ``x + noise_rate * normalize(noise[n_id])`` over one
    shared block and returns ``(h_pure, logp_pure, z_pure, h_noisy,
    logp_noisy, z_noisy)``: ``h`` the last hidden activation (after ReLU and
    ``bn2``, before dropout), ``z`` the logits, ``logp = log_softmax(z, 1)``.

    The noise add and its backward are one launch each
    (``ngnn.ops.add_node_noise``); every layer runs the per-conv path, whose
    layer 0 hands back the input gradient that trains the table.  State-dict
    keys are the reference's (``noise``, ``convs.{i}.lin_l.weight`` ...).

    ``fused_stack=True`` (opt-in) runs each pass as one autograd node on the
    fused per-layer kernels instead (``fused.sage_stack_tap``: ReLU and
    dropout in the layer epilogue, the receptive-field-bounded backward);
    ``use_bn=True`` and non-fp32 inputs keep the per-conv path.

    ``num_layers >= 2``: with one layer the reference's ``h`` is never
    assigned (sagePL.py:60 runs for hidden layers only) and its forward
    raises; here the constructor does.  The noise path is fp32 only.
    """

    def __init__(self, in_size, hidden_size, out_size, num_layers, nbr_nodes, dropout=0.5,
                 use_bn=False, aggr: str = "mean", fused_stack: bool = False):
        super().__init__()
        self.fused_stack = bool(fused_stack)
        if num_layers < 2:
            raise ValueError("SAGEPL needs num_layers >= 2: the hidden state it returns is the last "
                             "hidden layer's (undefined in the reference for one layer)")
        self.num_layers = num_layers
        self.dropout = dropout
        self.convs = nn.ModuleList()
        self.convs.append(SAGEConv(in_size, hidden_size, aggr=aggr))
        for _ in range(num_layers - 2):
            self.convs.append(SAGEConv(hidden_size, hidden_size, aggr=aggr))
        self.convs.append(SAGEConv(hidden_size, out_size, aggr=aggr))
        # adaptive noise to be added (sagePL.py:22)
        self.noise = nn.Parameter(torch.randn(nbr_nodes, in_size))
        self.use_bn = use_bn
        if self.use_bn:
            self.bn1 = nn.BatchNorm1d(in_size)
            self.bn2 = nn.BatchNorm1d(hidden_size)

    def reset_parameters(self):
        for conv in self.convs:  # (the convs only, as the reference: sagePL.py:29-31)
            conv.reset_parameters()

    def forward(self, x, edge_index, noise_rate=0.1, n_id=None):
        _refuse_sync_free(edge_index)
        if isinstance(x, IndexedRows):  # eager: gather the rows
            x = x.materialize()
        block = get_block(edge_index, x.size(0))  # built once, shared by both passes
        pure = self._stack(x, block)
        noisy_x = self.adding_noise(x, noise_rate=noise_rate, n_id=n_id)
        return pure + self._stack(noisy_x, block)

    def adding_noise(self, x, noise_rate, n_id=None):
        # n_id=None: the sign branch over the whole table (sagePL.py:43-44)
        return add_node_noise(x, self.noise, n_id=n_id, rate=noise_rate, sign=n_id is None)

    def _stack(self, x, block):
        if self.fused_stack and fused.sage_tap_supported(self, x):  # (excludes use_bn)
            z, h = fused.sage_stack_tap(self, x, block, *_dropout_seed(self, x, block), training=self.training)
            return h, torch.log_softmax(z, dim=1), z
        if self.use_bn:
            x = batch_norm_act(x, self.bn1)
        for i, conv in enumerate(self.convs):
            x = conv(x, block)
            if i != self.num_layers - 1:
                if self.use_bn:  # ReLU and BatchNorm in one op; h needs the value before dropout
                    x = batch_norm_act(x, self.bn2, relu=True)
                else:
                    x = x.relu()
                h = x
                x = F.dropout(x, p=self.dropout, training=self.training)
        return h, torch.log_softmax(x, dim=1), x

    def forward_pure(self, x, edge_index):
        _refuse_sync_free(edge_index)
        return self._stack(x, get_block(edge_index, x.size(0)))

    def forward_noisy(self, x, edge_index):
        _refuse_sync_free(edge_index)
        return self._stack(x, get_block(edge_index, x.size(0)))

    @torch.no_grad()
    def inference(self, x_all, subgraph_loader, device):
        """sagePL.py:78-94 semantics: the convs alone, the noise unused (same
        loop, and the same block-free plan, as SAGE.inference)."""
        return _inference(self.convs, self.num_layers, x_all, subgraph_loader, device)


def _inference(convs, num_layers, x_all, subgraph_loader, device):
    """The block-free plan (ngnn.infer) when the loader is an in-order ngnn
    NeighborLoader over every node and the model is fp32; the reference loop
    for everything else (generic iterables of batches, shuffled or permuted
    seeds, sharded or sync-free loaders)."""
    if infer.eligible(convs, x_all, subgraph_loader, device):
        return infer.fused_inference(convs, num_layers, x_all, subgraph_loader, device)
    out = _layerwise_inference(convs, num_layers, x_all, subgraph_loader, device)
    last_inference_plan[:] = ["loop"] * num_layers
    return out


def _layerwise_inference(convs, num_layers, x_all, subgraph_loader, device):
    out_device = x_all.device
    x_cur = x_all.to(device)
    for i in range(num_layers):
        xs = []
        for batch in subgraph_loader:
            n_id = batch.n_id.to(device)
            edge_index = batch.edge_index.to(device)
            x = convs[i](x_cur.index_select(0, n_id), edge_index)
            x = x[:batch.batch_size]
            if i != num_layers - 1:
                x = x.relu()
            xs.append(x)
        x_cur = torch.cat(xs, dim=0)
    return x_cur.to(out_device)


class NGNN(object):
    """src/models/model.py:10-69: builds ``self.network`` from ``module`` and an
    Adam optimiser (weight decay commented out in the reference, model.py:68-69)."""

    def __init__(self, in_size=100, hidden_size=128, out_size=47, num_layers=2, dropout=0.5,
                 lr=0.001, optimizer='adam', module='sage', nbr_nodes=1, use_bn=False, wd=0.0005,
                 aggr='mean', sagepl_fused=False, gcn_normalize=False):
        self.criterion = None
        self.score_func = None
        self.metric_name = None
        self.in_size, self.hidden_size, self.out_size = in_size, hidden_size, out_size
        self.num_layers, self.dropout, self.nbr_nodes = num_layers, dropout, nbr_nodes
        self.lr, self.wd = lr, wd
        self.optimizer = optimizer
        self.module = module
        self.use_bn = use_bn
        self.aggr = aggr
        self.gcn_normalize = gcn_normalize
        self.sagepl_fused = sagepl_fused
        self.init_network()
        self.init_optimizer()

    def init_network(self):
        if self.module == 'gcn':
            self.network = SimpleGCN(in_size=self.in_size, hidden_size=self.hidden_size,
                                     out_size=self.out_size, num_layers=self.num_layers,
                                     dropout=self.dropout, normalize=self.gcn_normalize)
        elif self.module == 'sage':
            self.network = SAGE(in_size=self.in_size, hidden_size=self.hidden_size,
                                out_size=self.out_size, num_layers=self.num_layers,
                                dropout=self.dropout, use_bn=self.use_bn, aggr=self.aggr)
        elif self.module == 'sagePL':  # model.py:57-63 (use_bn is not passed on there)
            self.network = SAGEPL(in_size=self.in_size, hidden_size=self.hidden_size,
                                  out_size=self.out_size, num_layers=self.num_layers,
                                  dropout=self.dropout, nbr_nodes=self.nbr_nodes, aggr=self.aggr,
                                  fused_stack=self.sagepl_fused)
        elif self.module == 'sageH':  # model.py:51-56
            self.network = SAGEH(in_size=self.in_size, hidden_size=self.hidden_size,
                                 out_size=self.out_size, num_layers=self.num_layers,
                                 dropout=self.dropout, aggr=self.aggr)
        else:
            raise ValueError(f"module {self.module!r} is outside this path "
                             "(supported: 'sage', 'sageH', 'sagePL', 'gcn'; see DESIGN.md scope)")

    def init_optimizer(self):
        if self.optimizer == 'adam':
            self.optimizer = torch.optim.Adam(self.network.parameters(), lr=self.lr)
        else:
            raise ValueError(f"optimizer {self.optimizer!r}: only 'adam' is reachable in the "
                             "reference (model.py:67-69; the other branches reference "
                             "undefined attributes)")
