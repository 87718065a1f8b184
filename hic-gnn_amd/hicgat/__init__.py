"""hicgat -- the GAT-HiC per-epoch hot path on MI355X (gfx950) HIP kernels.

Drop-in surface of the reference (beyzoskaya/HiC-GNN):
  hicgat.nn.GATConv                           ~ torch_geometric.nn.GATConv (PyG 1.7.2), dropout=p (on the
                                                attention coefficients) included
  hicgat.nn.SAGEConv                          ~ layers.SAGEConv (layers.py:12-79)
  hicgat.gat_models.GATNetSelectiveResidualsUpdated / GATNetHeadsChanged3LayersLeakyReLUv2 / Net
                                              ~ models.py:614-691 / :1010-1047 / :14-55
  hicgat.gat_models.GATNetHeadsChangedLeakyReLU / GATNetReduced (eval only)
                                              ~ models.py:181-222 / :1414-1459
  hicgat.gat_models.GATNet / GATNetHeadsChanged3LayersLeakyReLU /
      GATNetHeadsChanged4LayerEmbedding512Dense / GATNetMoreReduced (trained with feature dropout)
                                              ~ models.py:60-98 / :971-1007 / :1365-1411 / :1461-1494
  hicgat.gat_models.GATNetHeadsChanged4LayersLeakyReLU / GATNetHeadsChanged4LayersLeakyReLUHeads4
      (BatchNorm1d + feature dropout)         ~ models.py:270-319 / :834-883
  hicgat.gat_models.GATNetHeadsChanged3LayersEmbeddingDim256Entropy (attention weights + entropy term)
                                              ~ models.py:1112-1148
  hicgat.gat_models.LN_MODELS (six LayerNorm tails: ...ReLU_LayerNorm, ...LeakyReLU_LayerNorm, ...Embed512,
      ...Embed512WithResiduals, GATNetSelectiveResiduals, GATNetSelectiveResidualsUpdatedLayerNorm)
                                              ~ models.py:321-377 / :776-832 / :379-435 / :437-526 / :528-612 / :693-773
  hicgat.ops.ln_act_res / dual_ln_act_res     ~ torch.nn.LayerNorm -> relu / leaky_relu / gelu (+ residual)
                                                (-> torch.nn.LayerNorm)
  hicgat.ops.act                              ~ F.gelu / F.leaky_relu
  hicgat.ops.bn_act_dropout                   ~ torch.nn.BatchNorm1d -> F.leaky_relu -> torch.nn.Dropout(p)
  hicgat.ops.act_dropout, hicgat.DropoutState ~ x.relu() / F.leaky_relu(x) -> torch.nn.Dropout(p)
  hicgat.ops.attention_dropout_mask           ~ the keep mask of GATConv(dropout=p) (tests, tools)
  hicgat.ops.fused_dist_loss(kind="mse+pearson" | "rmse" | "si_mse", alpha=...)
                                              ~ mse_loss + alpha * (1 - r) with a gradient through r, rmse_loss,
                                                scale_invariant_mse (HiC_GAT_generalize_directly.py:60-68, :219-225)
  hicgat.graph.load_input / cont2dist / convert_to_matrix / Adj
                                              ~ utils.py:10-80 (+ torch_sparse.SparseTensor)
  hicgat.train.train / main                   ~ HiC-GNN_main.py:107-160
  hicgat.metrics.dscc, hicgat.io.write_pdb    ~ HiC-GNN_main.py:135-139, utils.WritePDB
  hicgat.kr.KRnorm                            ~ r_utils.R:1-93 (normalize.R)
  hicgat.align.domain_alignment / generalize  ~ utils.py:83-109, HiC_GAT_generalize_directly.py:312-336
  hicgat.embed.node2vec                       ~ Node2Vec(...).fit(...) at HiC_GAT_generalize_directly.py:150-155
  hicgat.embed.line                           ~ LINE(G, embedding_size=512, order='second').train(bs, ep) at
                                                HiC-GNN_main.py:91-96 (second order only)
Compute runs in libhicgat.so (include/hicgat.h); there is no CPU fallback.
"""
from . import (_lib, align, dist, dropout, embed, graph, graphs, io, kernels, kr, metrics, nn, ops, optim,  # noqa: F401
               paramgrads, synth, train)
from .dropout import DropoutState  # noqa: F401
from .gat_models import (GATNet, GATNetHeadsChanged3LayersEmbeddingDim256Entropy,  # noqa: F401
                         GATNetHeadsChanged3LayersLeakyReLU,
                         GATNetHeadsChanged3LayersLeakyReLUv2,
                         GATNetHeadsChanged4LayerEmbedding512Dense,
                         GATNetHeadsChanged4LayersLeakyReLU,
                         GATNetHeadsChanged4LayersLeakyReLUHeads4,
                         GATNetHeadsChangedLeakyReLU, GATNetMoreReduced, GATNetReduced,
                         GATNetSelectiveResidualsUpdated, MODELS, Net)
from .gat_models import (ALL_MODELS, LN_MODELS, GATNetHeadsChanged4LayersLeakyReLU_LayerNorm,  # noqa: F401
                         GATNetHeadsChanged4LayersReLU_LayerNorm,
                         GATNetHeadsChanged4LayersReLU_LayerNormEmbed512,
                         GATNetHeadsChanged4LayersReLU_LayerNormEmbed512WithResiduals,
                         GATNetSelectiveResiduals, GATNetSelectiveResidualsUpdatedLayerNorm)
from .graph import Adj, Data, Truth, cont2dist, convert_to_matrix, load_input  # noqa: F401
from .nn import GATConv, SAGEConv  # noqa: F401
from .optim import FlatAdam  # noqa: F401

__version__ = "0.1.0"
