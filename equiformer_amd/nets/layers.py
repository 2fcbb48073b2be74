"""Building blocks of the graph-attention transformer on top of the HIP operators.

Module and parameter names reproduce the reference's state_dict: `*.tp.weight` (flat, e3nn
instruction order), `*.bias.0`, `*.dtp_rad.net.{0,1,3,4,6}.*`, `*.dtp_rad.offset`, `norm_*.affine_{weight,bias}`...
Reference sources of the semantics (paths relative to the reference root):
  nets/tensor_product_rescale.py:15-174   TensorProductRescale / FullyConnectedTensorProductRescale / LinearRS
  nets/fast_activation.py:15-160          Activation / Gate
  nets/layer_norm.py:62-152               EquivariantLayerNormV2
  nets/graph_norm.py:9-134                EquivariantGraphNorm
  nets/instance_norm.py:9-134             EquivariantInstanceNorm
  nets/fast_layer_norm.py                 EquivariantLayerNormFast
  nets/radial_func.py:9-49                RadialProfile
  nets/gaussian_rbf.py:13-40              GaussianRadialBasisLayer
  nets/graph_attention_transformer.py     DepthwiseTensorProduct :157, SeparableFCTP :186, GraphAttention :403,
                                          FeedForwardNetwork :537, TransBlock :575, NodeEmbeddingNetwork :670,
                                          ScaledScatter :693, EdgeDegreeEmbeddingNetwork :709
"""
import math
import os

import torch
from torch import nn

from .. import droppath, ops, so3
from ..dropout import EquivariantDropout
from ..irreps import Irrep, Irreps
from ..layout import DtpTable, RowLayout

_RESCALE = True
_USE_BIAS = True


def _simplified_sorted(irreps):
    irreps = Irreps(irreps)
    s, _ = irreps.sort_even_first()
    return s.simplify()


class _TensorProductWeights(nn.Module):
    """Stands where e3nn's `o3.TensorProduct` sits in the reference module tree (`<module>.tp`): owns the flat
    `weight` (a Parameter when internal, an empty buffer otherwise, as e3nn registers it)."""

    def __init__(self, weight_numel, internal):
        super().__init__()
        self.weight_numel = weight_numel
        self.internal_weights = internal
        if internal and weight_numel > 0:
            self.weight = nn.Parameter(torch.randn(weight_numel))
        else:
            self.register_buffer("weight", torch.Tensor())


def irreps2gate(irreps):
    irreps = Irreps(irreps)
    scalars = Irreps([(m, ir) for m, ir in irreps if ir.l == 0 and ir.p == 1]).simplify()
    gated = Irreps([(m, ir) for m, ir in irreps if not (ir.l == 0 and ir.p == 1)]).simplify()
    gates = Irreps([(m, Irrep(0, 1)) for m, _ in gated]).simplify() if gated.dim > 0 else Irreps()
    return scalars, gates, gated


class FullyConnectedTensorProductRescale(nn.Module):
    """FCTP(irreps_in1 x '1x0e' -> irreps_out): with a scalar second operand every path is a per-degree dense
    channel mix out_l = x_l W_l (+ bias on 0e), executed as MFMA GEMMs on the l-segments of the rows."""

    def __init__(self, irreps_in1, irreps_in2, irreps_out, bias=True, rescale=True, internal_weights=None,
                 shared_weights=None, normalization=None):
        super().__init__()
        self.irreps_in1 = Irreps(irreps_in1)
        self.irreps_in2 = Irreps(irreps_in2)
        self.irreps_out = Irreps(irreps_out)
        if self.irreps_in2 != Irreps("1x0e"):
            raise NotImplementedError("only scalar node attributes ('1x0e') are supported, got %r" % self.irreps_in2)
        self.rescale, self.use_bias = rescale, bias
        self.layout_in = RowLayout(self.irreps_in1) if self._is_layout(self.irreps_in1) else RowLayout(
            self.irreps_in1.simplify())
        self.layout_out = RowLayout(self.irreps_out.simplify())
        self.spec = ops.LinearSpec(self.layout_in, self.layout_out)
        self.tp = _TensorProductWeights(self.spec.weight_numel, True)
        biases = []
        if bias and self.spec.bias_dim > 0:
            biases.append(nn.Parameter(torch.zeros(self.spec.bias_dim)))
        self.bias = nn.ParameterList(biases)
        if rescale:
            with torch.no_grad():
                for (l, _, K, _, N, w_off) in self.spec.pairs:
                    self.tp.weight[w_off:w_off + K * N].mul_(1.0 / math.sqrt(K))

    @staticmethod
    def _is_layout(irreps):
        keys = [(ir.l, -ir.p) for _, ir in irreps]
        return keys == sorted(set(keys))

    def _bias(self):
        return self.bias[0] if len(self.bias) > 0 else None

    def forward_tp_rescale_bias(self, x, y=None, weight=None):
        return ops.irreps_linear(x, self.tp.weight, self._bias(), self.spec)

    def forward(self, x, y=None, weight=None):
        return self.forward_tp_rescale_bias(x, y, weight)


class LinearRS(FullyConnectedTensorProductRescale):
    def __init__(self, irreps_in, irreps_out, bias=True, rescale=True):
        super().__init__(irreps_in, Irreps("1x0e"), irreps_out, bias=bias, rescale=rescale, internal_weights=True,
                         shared_weights=True)

    def forward(self, x):
        return self.forward_tp_rescale_bias(x)


class Activation(nn.Module):
    """Second-moment-normalised scalar activation applied to a whole 0e tensor (fast_activation.py:68-71)."""

    def __init__(self, irreps_in, acts=None, kind="silu"):
        super().__init__()
        self.irreps_in = self.irreps_out = Irreps(irreps_in)
        assert all(ir.l == 0 and ir.p == 1 for _, ir in self.irreps_in)  # SiLU is neither even nor odd: 0e only
        self.kind = kind
        self.cst = {"silu": so3.C_SILU}[kind]

    def forward(self, x):
        return ops.scaled_silu(x, self.cst)


class Gate(nn.Module):
    def __init__(self, irreps_scalars, irreps_gates, irreps_gated):
        super().__init__()
        self.irreps_scalars, self.irreps_gates, self.irreps_gated = irreps_scalars, irreps_gates, irreps_gated
        self._irreps_in = (irreps_scalars + irreps_gates + irreps_gated).simplify()
        self._irreps_out = (irreps_scalars + irreps_gated).simplify()
        self.S = irreps_scalars.dim
        self.gated_layout = RowLayout(irreps_gated)

    @property
    def irreps_in(self):
        return self._irreps_in

    @property
    def irreps_out(self):
        return self._irreps_out

    def forward(self, x):
        return ops.gate(x, self.S, self.gated_layout, so3.C_SILU, so3.C_SIGMOID)


def make_gate(irreps_out):
    scalars, gates, gated = irreps2gate(irreps_out)
    if gated.num_irreps == 0:
        return Activation(irreps_out, kind="silu")
    return Gate(scalars, gates, gated)


class FullyConnectedTensorProductRescaleSwishGate(FullyConnectedTensorProductRescale):
    def __init__(self, irreps_in1, irreps_in2, irreps_out, bias=True, rescale=True, internal_weights=None,
                 shared_weights=None, normalization=None):
        gate = make_gate(irreps_out)
        super().__init__(irreps_in1, irreps_in2, gate.irreps_in, bias=bias, rescale=rescale)
        self.gate = gate

    def forward(self, x, y=None, weight=None):
        return self.gate(self.forward_tp_rescale_bias(x, y, weight))


class EquivariantLayerNormV2(nn.Module):
    def __init__(self, irreps, eps=1e-5, affine=True, normalization="component"):
        super().__init__()
        assert affine and normalization == "component"
        self.irreps = Irreps(irreps)
        self.layout = RowLayout(self.irreps.simplify())
        self.eps = eps
        self.affine_weight = nn.Parameter(torch.ones(self.irreps.num_irreps))
        self.affine_bias = nn.Parameter(torch.zeros(sum(m for m, ir in self.irreps if ir.l == 0 and ir.p == 1)))

    def forward(self, node_input, graph=None, **kwargs):
        _check_row(node_input, self.layout)
        return ops.layer_norm(node_input, self.affine_weight, self.affine_bias, self.layout, self.eps)

    def forward_sum(self, a, b, graph=None):
        """(a + b, norm(a + b)) in one launch: the residual add that precedes every norm of the transformer.  `graph` (what
        the per-graph norms below need) is accepted and ignored."""
        _check_row(a, self.layout)
        return ops.add_layer_norm(a, b, self.affine_weight, self.affine_bias, self.layout, self.eps)

    def __repr__(self):
        return "{}({}, eps={})".format(self.__class__.__name__, self.irreps, self.eps)


def _check_row(x, layout):
    if x.shape[-1] != layout.dim:
        raise AssertionError("`ix` should have reached node_input.size(-1) ({}), but it ended at {}".format(
            x.shape[-1], layout.dim))


class EquivariantLayerNormFast(nn.Module):
    """[ref: nets/fast_layer_norm.py] the reference's second formulation of the layer norm: the same function of the same
    parameters as EquivariantLayerNormV2 (2e-15 apart in fp64), so it runs on the same kernels.  A class of its own, NOT a
    subclass of V2: the reference's no_weight_decay() does not list it, and the mirror here must not either."""

    def __init__(self, irreps, eps=1e-5, affine=True, normalization="component"):
        super().__init__()
        if not affine or normalization != "component":
            raise NotImplementedError("EquivariantLayerNormFast: only affine=True, normalization='component' is built")
        self.irreps = Irreps(irreps)
        self.layout = RowLayout(self.irreps.simplify())
        self.eps = eps
        self.affine_weight = nn.Parameter(torch.ones(self.irreps.num_irreps))
        self.affine_bias = nn.Parameter(torch.zeros(sum(m for m, ir in self.irreps if ir.l == 0 and ir.p == 1)))

    def forward(self, node_input, graph=None, **kwargs):
        _check_row(node_input, self.layout)
        return ops.layer_norm(node_input, self.affine_weight, self.affine_bias, self.layout, self.eps)

    def forward_sum(self, a, b, graph=None):
        _check_row(a, self.layout)
        return ops.add_layer_norm(a, b, self.affine_weight, self.affine_bias, self.layout, self.eps)

    def __repr__(self):
        return "{}({}, eps={})".format(self.__class__.__name__, self.irreps, self.eps)


class _PerGraphNorm(nn.Module):
    """What EquivariantGraphNorm and EquivariantInstanceNorm share: statistics per (graph, channel) over the nodes of a graph
    (ops.graph_norm; csrc/graphnorm.hip).  Only the defaults every model uses are built."""

    def __init__(self, irreps, eps=1e-5, affine=True, reduce="mean", normalization="component"):
        super().__init__()
        assert isinstance(reduce, str), "reduce should be passed as a string value"
        assert reduce in ["mean", "max"], "reduce needs to be 'mean' or 'max'"
        assert normalization in ["norm", "component"], "normalization needs to be 'norm' or 'component'"
        if not affine or reduce != "mean" or normalization != "component":
            raise NotImplementedError("{}: only affine=True, reduce='mean', normalization='component' is built (got "
                                      "affine={}, reduce={!r}, normalization={!r})".format(
                                          self.__class__.__name__, affine, reduce, normalization))
        self.irreps = Irreps(irreps)
        self.layout = RowLayout(self.irreps.simplify())
        self.eps, self.affine, self.reduce, self.normalization = eps, affine, reduce, normalization
        self._register(self.irreps.num_irreps, sum(m for m, ir in self.irreps if ir.l == 0 and ir.p == 1))

    def _mean_shift(self):
        return None  # the instance norm has no such parameter (= 1)

    def forward(self, node_input, graph=None, **kwargs):
        _check_row(node_input, self.layout)
        return ops.graph_norm(node_input, self._mean_shift(), self.affine_weight, self.affine_bias, self.layout, graph,
                              self.eps)

    def forward_sum(self, a, b, graph=None):
        """(a + b, norm(a + b)): the residual add rides on the norm's kernels."""
        _check_row(a, self.layout)
        return ops.add_graph_norm(a, b, self._mean_shift(), self.affine_weight, self.affine_bias, self.layout, graph,
                                  self.eps)

    def __repr__(self):
        return "{} ({}, eps={})".format(self.__class__.__name__, self.irreps, self.eps)


class EquivariantGraphNorm(_PerGraphNorm):
    """[ref: nets/graph_norm.py:9-134] parameters in the reference's order: mean_shift, affine_weight, affine_bias."""

    def _register(self, num_features, num_scalar):
        self.mean_shift = nn.Parameter(torch.ones(num_scalar))
        self.affine_weight = nn.Parameter(torch.ones(num_features))
        self.affine_bias = nn.Parameter(torch.zeros(num_scalar))

    def _mean_shift(self):
        return self.mean_shift


class EquivariantInstanceNorm(_PerGraphNorm):
    """[ref: nets/instance_norm.py:9-134] the graph norm without the mean shift."""

    def _register(self, num_features, num_scalar):
        self.affine_weight = nn.Parameter(torch.ones(num_features))
        self.affine_bias = nn.Parameter(torch.zeros(num_scalar))


def get_norm_layer(norm_type):
    if norm_type == "graph":
        return EquivariantGraphNorm
    if norm_type == "instance":
        return EquivariantInstanceNorm
    if norm_type == "layer":
        return EquivariantLayerNormV2
    if norm_type == "fast_layer":
        return EquivariantLayerNormFast
    if norm_type is None:
        return None
    raise ValueError("Norm type {} not supported.".format(norm_type))


class RadialProfile(nn.Module):
    """Linear -> LayerNorm -> SiLU (x2) -> Linear(no bias) + offset; parameters live in ordinary nn.Linear /
    nn.LayerNorm containers (so name-based weight-decay rules see the same types), compute is HIP."""

    def __init__(self, ch_list, use_layer_norm=True, use_offset=True):
        super().__init__()
        assert use_layer_norm and use_offset
        mods = []
        for i in range(1, len(ch_list)):
            last = i == len(ch_list) - 1
            mods.append(nn.Linear(ch_list[i - 1], ch_list[i], bias=not last))
            if last:
                break
            mods.append(nn.LayerNorm(ch_list[i]))
            mods.append(nn.SiLU())
        self.net = nn.Sequential(*mods)
        self.offset = nn.Parameter(torch.zeros(ch_list[-1]))
        bound = 1 / math.sqrt(ch_list[-2])
        nn.init.uniform_(self.offset, -bound, bound)

    def forward(self, f_in, hidden_only=False):
        """hidden_only: stop in front of the last layer (its consumer folds that layer into its own weights)"""
        x = f_in
        mods = list(self.net)
        i = 0
        while i < len(mods):
            lin = mods[i]
            if i == len(mods) - 1:
                return x if hidden_only else ops.dense_linear(x, lin.weight, self.offset)  # y = x W^T + offset
            ln = mods[i + 1]
            x = ops.dense_linear(x, lin.weight, lin.bias)
            x = ops.ln_silu(x, ln.weight, ln.bias, ln.eps)
            i += 3
        return x


class RadialBank:
    """All RadialProfile MLPs of a model (one per transformer block + the edge-degree embedding) evaluated side by side
    on the shared radial basis: every one of them maps the SAME edge_length_embedding through Linear-LN-SiLU-Linear-LN-
    SiLU-Linear (+offset) with its own parameters [ref: nets/graph_attention_transformer.py:200-208,445-447,717;
    forward :880-886].  Per module that is 5 launches forward and 10 backward on tensors of only 64 columns; side by
    side it is ONE 128 -> G*64 GEMM, two grouped LayerNorm+SiLU launches and two grouped-GEMM launches for all G
    modules (eqf_gemm_group / eqf_lnsilu_group_*), forward and backward alike.  A plain helper object: the parameters
    stay where the reference's state_dict has them."""

    def __init__(self, modules):
        self.modules = [m for m in modules if m is not None]
        mods = [list(m.net) for m in self.modules]
        self.ok = len(self.modules) >= 2 and all(
            len(ms) == 7 and ms[0].weight.shape == mods[0][0].weight.shape and ms[3].weight.shape == mods[0][3].weight.shape
            and ms[3].weight.shape[0] == ms[3].weight.shape[1] and ms[0].weight.shape[0] <= 64 for ms in mods)

    # The LAST layer (64 -> weight_numel, 960 for the QM9 model) all G modules at once writes 681 MB at the bench size (E = 25 354),
    # long before its consumers run and far beyond the 256 MB infinity cache.  Round 6 measured the alternative asked for by the
    # round-5 review -- each module's last layer when its block asks for the weights (immediately before the block's sfcx forward,
    # its backward immediately after the block's data gradient, so that w / dw are produced and consumed inside the cache;
    # EQF_RADIAL_LAST_BANKED=0): the step got SLOWER, 10.08 ms against 9.68-9.71 ms on the same box, twice
    # (profiles/r06/r06_r_unbank_radial_last_layer_ab.txt) -- seven single-module launches per direction (and fourteen in the
    # backward) cost more than the grouped ones save in HBM reads.  The banked form stays the default.
    LAST_BANKED = os.environ.get("EQF_RADIAL_LAST_BANKED", "1") == "1"

    def forward(self, edge_scalars, hidden_only=()):
        """-> {id(module): [E, weight_numel]} (LAST_BANKED) or {id(module): hidden activation [E, 64] of the module's last layer}.
        The modules in `hidden_only` are left out of the grouped last layer (their consumer wants the hidden activation: the
        collapsed edge-degree embedding) and get their hidden activation whatever LAST_BANKED says."""
        ms = self.modules
        G = len(ms)
        C = ms[0].net[0].weight.shape[0]
        cat = torch.cat
        h = ops.dense_linear(edge_scalars, cat([m.net[0].weight for m in ms]), cat([m.net[0].bias for m in ms]))
        h = ops.ln_silu(h, cat([m.net[1].weight for m in ms]), cat([m.net[1].bias for m in ms]), ms[0].net[1].eps, groups=G)
        h = ops.grouped_linear(h, C, [m.net[3].weight for m in ms], [m.net[3].bias for m in ms], wide=True)
        h = ops.ln_silu(h, cat([m.net[4].weight for m in ms]), cat([m.net[4].bias for m in ms]), ms[0].net[4].eps, groups=G)
        if self.LAST_BANKED:
            hid = {id(m) for m in hidden_only}
            cols = [g for g, m in enumerate(ms) if id(m) not in hid]
            rest = [m for m in ms if id(m) in hid]
            if not rest:
                outs = ops.grouped_linear(h, C, [m.net[6].weight for m in ms], [m.offset for m in ms], wide=False)
                return {id(m): o for m, o in zip(ms, outs)}
            if not cols:
                return {id(m): hg for m, hg in zip(ms, ops.split_columns(h, G))}
            last = [ms[g] for g in cols]
            outs = ops.grouped_linear(h, C, [m.net[6].weight for m in last], [m.offset for m in last], wide=False, cols=cols)
            return {id(m): o for m, o in zip(last + rest, outs)}
        return {id(m): hg for m, hg in zip(ms, ops.split_columns(h, G))}

    @staticmethod
    def last_layer(module, hidden):
        return ops.dense_linear(hidden, module.net[6].weight, module.offset)  # y = h W^T + offset


class GaussianRadialBasisLayer(nn.Module):
    def __init__(self, num_basis, cutoff):
        super().__init__()
        self.num_basis, self.cutoff = num_basis, cutoff + 0.0
        self.mean = nn.Parameter(torch.zeros(1, num_basis))
        self.std = nn.Parameter(torch.zeros(1, num_basis))
        self.weight = nn.Parameter(torch.ones(1, 1))
        self.bias = nn.Parameter(torch.zeros(1, 1))
        nn.init.uniform_(self.mean, 0, 1.0)
        nn.init.uniform_(self.std, 1.0 / num_basis, 1.0)

    def forward(self, dist, node_atom=None, edge_src=None, edge_dst=None):
        return ops.rbf_gaussian(dist, self.mean, self.std, self.weight, self.bias, self.cutoff)


class ExpNormalSmearing(nn.Module):
    """[ref: nets/graph_attention_transformer_md17.py:85-124], non-trainable buffers `means`, `betas`."""

    def __init__(self, cutoff_lower=0.0, cutoff_upper=5.0, num_rbf=50, trainable=False):
        super().__init__()
        assert cutoff_lower == 0.0 and not trainable
        self.cutoff_lower, self.cutoff_upper, self.num_rbf = cutoff_lower, cutoff_upper, num_rbf
        self.alpha = 5.0 / (cutoff_upper - cutoff_lower)
        start = torch.exp(torch.scalar_tensor(-cutoff_upper + cutoff_lower))
        self.register_buffer("means", torch.linspace(start, 1, num_rbf))
        self.register_buffer("betas", torch.tensor([(2 / num_rbf * (1 - start)) ** -2] * num_rbf))

    def forward(self, dist):
        return ops.rbf_expnorm(dist, self.means, self.betas, self.alpha, self.cutoff_upper)


class SphericalBesselBasis(nn.Module):
    """Holds `frequencies` under the reference's key `rbf.rbf.frequencies` (ocpmodels gemnet/layers/radial_basis.py)."""

    def __init__(self, num_radial, cutoff):
        super().__init__()
        self.frequencies = nn.Parameter(torch.tensor([math.pi * k for k in range(1, num_radial + 1)], dtype=torch.float32))


class RadialBasis(nn.Module):
    """ocpmodels' RadialBasis(num_radial, cutoff, rbf={'name': 'spherical_bessel'}) with the default polynomial
    envelope (exponent 5) [ref call sites: nets/graph_attention_transformer.py:786-788, ..._md17.py:178-180]; the
    arithmetic is `eqf_rbf_bessel_*` (csrc/graph.hip)."""

    def __init__(self, num_radial, cutoff, rbf=None, envelope=None):
        super().__init__()
        name = (rbf or {"name": "spherical_bessel"}).get("name")
        if name != "spherical_bessel" or (envelope or {"exponent": 5}).get("exponent", 5) != 5:
            raise NotImplementedError("only the spherical-Bessel basis with the exponent-5 envelope is on the hot path")
        self.cutoff = float(cutoff)
        self.rbf = SphericalBesselBasis(num_radial, cutoff)

    def forward(self, dist, *unused):
        return ops.rbf_bessel(dist, self.rbf.frequencies, self.cutoff)


# ------------------------------------------------------------------------------------------------- edge context
class EdgeContext:
    """Per-forward geometry shared by every block: the dst-sorted graph, spherical harmonics, radial basis and
    the DTP coupling matrices (one tensor per distinct path table, computed once per forward)."""

    def __init__(self, graph, edge_sh, edge_scalars, radial_bank=None, hidden_only=()):
        """hidden_only: RadialProfile modules whose consumer asks for `radial_hidden` instead of `radial`"""
        self.graph, self.edge_sh, self.edge_scalars = graph, edge_sh, edge_scalars
        self._coupling = {}
        self._bank, self._radial = radial_bank, None
        self._hidden_only = tuple(hidden_only)

    def _banked(self, module):
        if self._bank is None:
            return None
        if self._radial is None:
            self._radial = self._bank.forward(self.edge_scalars, self._hidden_only)
        return self._radial.get(id(module))

    def wants_hidden(self, module):
        return any(m is module for m in self._hidden_only)

    def radial(self, module):
        """Per-edge path weights of `module` (a RadialProfile): from the model's radial bank when there is one (all
        modules evaluated together on first use), otherwise the module on its own."""
        w = self._banked(module)
        if w is not None:
            if self._bank.LAST_BANKED and not self.wants_hidden(module):
                return w
            return self._bank.last_layer(module, w)
        return module(self.edge_scalars)

    def radial_hidden(self, module):
        """Hidden activation [E, 64] in front of the last layer of `module`, which must have been named in `hidden_only`: from
        the bank (which then leaves the module's last layer out of its grouped launch), otherwise the module's own layers."""
        assert self.wants_hidden(module)
        h = self._banked(module)
        return h if h is not None else module(self.edge_scalars, hidden_only=True)

    def coupling(self, table):
        c = self._coupling.get(table.key)
        if c is None:
            c = ops.dtp_coupling(self.edge_sh, table)
            self._coupling[table.key] = c
        return c


class DepthwiseTensorProductModule(nn.Module):
    """Holds the path table (+ internal weights when shared); `tp` keeps the reference's key `dtp.tp.weight`."""

    def __init__(self, irreps_node_input, irreps_edge_attr, irreps_node_output, internal_weights=False, bias=True):
        super().__init__()
        assert not bias
        self.table = DtpTable(irreps_node_input, irreps_edge_attr, irreps_node_output)
        self.irreps_out = self.table.irreps_out_unsimplified
        self.tp = _TensorProductWeights(self.table.weight_numel, internal_weights)
        # 'uvu' with mul2 == 1: fan_in = 1 -> rescale factor 1 (tensor_product_rescale.py:46,93-110)
        self.slices_sqrt_k = {}


def DepthwiseTensorProduct(irreps_node_input, irreps_edge_attr, irreps_node_output, internal_weights=False, bias=True):
    return DepthwiseTensorProductModule(irreps_node_input, irreps_edge_attr, irreps_node_output,
                                        internal_weights=internal_weights, bias=bias)


class SeparableFCTP(nn.Module):
    def __init__(self, irreps_node_input, irreps_edge_attr, irreps_node_output, fc_neurons, use_activation=False,
                 norm_layer=None, internal_weights=False):
        super().__init__()
        assert norm_layer is None
        self.irreps_node_input = Irreps(irreps_node_input)
        self.irreps_edge_attr = Irreps(irreps_edge_attr)
        self.irreps_node_output = Irreps(irreps_node_output)
        self.dtp = DepthwiseTensorProduct(self.irreps_node_input, self.irreps_edge_attr, self.irreps_node_output,
                                          bias=False, internal_weights=internal_weights)
        self.dtp_rad = None
        if fc_neurons is not None:
            self.dtp_rad = RadialProfile(fc_neurons + [self.dtp.tp.weight_numel])
        irreps_lin_output = self.irreps_node_output
        if use_activation:
            s, g, gd = irreps2gate(self.irreps_node_output)
            irreps_lin_output = (s + g + gd).simplify()
        self.lin = LinearRS(self.dtp.table.irreps_out, irreps_lin_output)
        self.norm = None
        self.gate = make_gate(self.irreps_node_output) if use_activation else None
        self.fused_spec = ops.DtpLinearSpec.make(self.dtp.table, self.lin.layout_out)
        self.sfc_spec = ops.SfcSpec(self.dtp.table, self.lin.layout_out)
        if internal_weights:
            # row (path, channel) of the stacked lin weight -> index of its shared DTP weight
            idx = []
            t = self.dtp.table
            for k3 in sorted({(p["l3"], -p["p3"]) for p in t.paths}):
                for p in t.paths:
                    if (p["l3"], -p["p3"]) == k3:
                        idx.extend(range(p["w_off"], p["w_off"] + p["mul"]))
            self.register_buffer("_row_to_w", torch.tensor(idx, dtype=torch.long), persistent=False)
            # element of the flat lin weight -> index of the shared DTP weight scaling its row
            elem, r = [], 0
            for (l, _, K, _, N, w_off) in self.lin.spec.pairs:
                for k in range(K):
                    elem.extend([idx[r + k]] * N)
                r += K
            self.register_buffer("_elem_to_w", torch.tensor(elem, dtype=torch.long), persistent=False)
            # rows of the flat lin weight: first element of every row and the shared weight that scales it (eqf_fold_weight_*)
            starts, o = [], 0
            for (l, _, K, _, N, w_off) in self.lin.spec.pairs:
                assert w_off == o
                starts.extend(range(o, o + K * N, N))
                o += K * N
            starts.append(o)
            # eqf_fold_weight_* pair row r of the flat lin weight with shared weight idx[r] and WRITE dw[idx[r]] (no
            # accumulation): rows and shared weights must correspond one to one (every DTP output segment has its pair)
            assert len(starts) - 1 == len(idx) and len(set(idx)) == len(idx), (len(starts) - 1, len(idx))
            self.register_buffer("_row_start", torch.tensor(starts, dtype=torch.int32), persistent=False)
            self.register_buffer("_w_of_row", torch.tensor(idx, dtype=torch.int32), persistent=False)

    def folded_lin_weight(self):
        """lin weight with the shared depth-wise weights folded into its rows:
        Linear(DTP_w(x)) == Linear'(DTP_1(x)) with W'[(p,u), :] = w[p,u] * W[(p,u), :]."""
        scale = self.dtp.tp.weight.index_select(0, self._row_to_w)
        chunks, r = [], 0
        for (l, _, K, _, N, w_off) in self.lin.spec.pairs:
            W = self.lin.tp.weight[w_off:w_off + K * N].view(K, N)
            chunks.append((W * scale[r:r + K, None]).reshape(-1))
            r += K
        return torch.cat(chunks)

    def flat_weight(self):
        """Flat lin weight ([K(l), N(l)] blocks, ascending degree) with the shared depth-wise weights
        (internal_weights=True) folded into the rows: two element-wise kernels instead of per-degree slicing."""
        if self.dtp.tp.internal_weights:
            # index_select, not weight[idx]: the backward of advanced indexing is index_put_(accumulate=True), which
            # sorts the 64 512 indices on the device (45 rocPRIM launches per block); index_select's is one index_add_
            if self.lin.tp.weight.is_cuda:
                return ops.fold_weight(self.lin.tp.weight, self.dtp.tp.weight, self._row_start, self._w_of_row)
            return self.lin.tp.weight * self.dtp.tp.weight.index_select(0, self._elem_to_w)
        return self.lin.tp.weight

    def forward(self, node_input, ectx, use_fused=True):
        table = self.dtp.table
        M = ectx.coupling(table)
        internal = self.dtp.tp.internal_weights
        w = ectx.radial(self.dtp_rad) if self.dtp_rad is not None else None
        bias = self.lin._bias()
        if use_fused is True and self.sfc_spec.supported:
            out = ops.sep_fctp(node_input, M, w, self.flat_weight(), bias, self.sfc_spec)
        elif use_fused and self.fused_spec is not None:
            weight = self.folded_lin_weight() if internal else self.lin.tp.weight
            out = ops.dtp_linear(node_input, M, w, weight, bias, self.fused_spec)
        else:
            if internal:
                w = self.dtp.tp.weight.unsqueeze(0).expand(node_input.shape[0], -1).contiguous()
            out = self.lin(ops.dtp(node_input, M, w, table))
        if self.gate is not None:
            out = self.gate(out)
        return out


class GraphAttention(nn.Module):
    def __init__(self, irreps_node_input, irreps_node_attr, irreps_edge_attr, irreps_node_output, fc_neurons,
                 irreps_head, num_heads, irreps_pre_attn=None, rescale_degree=False, nonlinear_message=False,
                 alpha_drop=0.1, proj_drop=0.1):
        super().__init__()
        self.irreps_node_input = Irreps(irreps_node_input)
        self.irreps_node_attr = Irreps(irreps_node_attr)
        self.irreps_edge_attr = Irreps(irreps_edge_attr)
        self.irreps_node_output = Irreps(irreps_node_output)
        self.irreps_pre_attn = self.irreps_node_input if irreps_pre_attn is None else Irreps(irreps_pre_attn)
        self.irreps_head = Irreps(irreps_head)
        self.num_heads = num_heads
        self.rescale_degree = rescale_degree
        self.nonlinear_message = nonlinear_message
        if rescale_degree:
            raise NotImplementedError("rescale_degree=True is not used by any registered model")

        self.merge_src = LinearRS(self.irreps_node_input, self.irreps_pre_attn, bias=True)
        self.merge_dst = LinearRS(self.irreps_node_input, self.irreps_pre_attn, bias=False)

        irreps_attn_heads = _simplified_sorted(self.irreps_head * num_heads)
        mul_alpha = sum(m for m, ir in irreps_attn_heads if ir.l == 0 and ir.p == 1)
        self.mul_alpha_head = mul_alpha // num_heads
        irreps_alpha = Irreps("{}x0e".format(mul_alpha))

        if nonlinear_message:
            self.sep_act = SeparableFCTP(self.irreps_pre_attn, self.irreps_edge_attr, self.irreps_pre_attn, fc_neurons,
                                         use_activation=True, norm_layer=None, internal_weights=False)
            self.sep_alpha = LinearRS(self.sep_act.dtp.table.irreps_out, irreps_alpha)
            self.sep_value = SeparableFCTP(self.irreps_pre_attn, self.irreps_edge_attr, irreps_attn_heads,
                                           fc_neurons=None, use_activation=False, norm_layer=None,
                                           internal_weights=True)
            self.alpha_fused_spec = ops.DtpLinearSpec.make(self.sep_act.dtp.table, self.sep_alpha.layout_out)
            # value linear + attention-logit linear share ONE generation of the DTP output (concatenated degree-0
            # weight)
            self.act_sfc_spec = ops.SfcSpec(self.sep_act.dtp.table, self.sep_act.lin.layout_out, n2=mul_alpha)
        else:
            # linear messages [ref: nets/graph_attention_transformer.py:459-465,497-502]: ONE SeparableFCTP whose
            # output irreps are (alpha scalars + head irreps).simplify(); Vec2AttnHeads then cuts the scalar segment
            # into per-head runs [alpha (mul_alpha_head) | value scalars].  The same fused kernel serves it: the
            # columns of the degree-0 weight are split into the value part (main consumer) and the alpha part (second
            # consumer), a gather on a [K, 256] parameter per call instead of a permutation of per-edge data.
            irreps_attn_all = _simplified_sorted(irreps_alpha + irreps_attn_heads)
            self.sep = SeparableFCTP(self.irreps_pre_attn, self.irreps_edge_attr, irreps_attn_all, fc_neurons,
                                     use_activation=False, norm_layer=None, internal_weights=False)
            n0 = sum(m for m, ir in irreps_attn_all if ir.l == 0 and ir.p == 1)
            hw = n0 // num_heads
            mah = self.mul_alpha_head
            self.register_buffer("_idx_alpha", torch.tensor([h * hw + k for h in range(num_heads) for k in range(mah)],
                                                            dtype=torch.long), persistent=False)
            self.register_buffer("_idx_value", torch.tensor([h * hw + mah + k for h in range(num_heads)
                                                             for k in range(hw - mah)], dtype=torch.long),
                                 persistent=False)
            self.lin_sfc_spec = ops.SfcSpec(self.sep.dtp.table, RowLayout(irreps_attn_heads), n2=mul_alpha)
            if not self.lin_sfc_spec.supported:
                raise NotImplementedError("linear-message attention needs the fused SeparableFCTP kernels "
                                          "(channel counts in multiples of 32)")
        self.heads_layout = RowLayout(irreps_attn_heads)

        self.alpha_dot = nn.Parameter(torch.randn(1, num_heads, self.mul_alpha_head))
        stdv = math.sqrt(6.0 / (self.alpha_dot.size(-2) + self.alpha_dot.size(-1)))  # torch_geometric glorot
        self.alpha_dot.data.uniform_(-stdv, stdv)
        self.alpha_drop = float(alpha_drop)
        self.alpha_dropout = nn.Dropout(alpha_drop) if alpha_drop != 0.0 else None  # marker module (no params)
        self.proj = LinearRS(irreps_attn_heads, self.irreps_node_output)
        # [ref: :476-479] the reference sizes the dropout with irreps_node_input: the same irreps in every block.  Where they
        # differ (an attention head built with proj_drop != 0: the MD17 / DeNS heads) its product with the projected rows
        # fails on the shapes; here the dropout is sized with the rows it multiplies.
        self.proj_drop = EquivariantDropout(self.irreps_node_output, proj_drop) if proj_drop != 0.0 else None
        self.use_fused = True

    def forward(self, node_input, node_attr=None, edge_src=None, edge_dst=None, edge_attr=None, edge_scalars=None,
                batch=None, ectx=None, **kwargs):
        g = ectx.graph
        # merge_src / merge_dst read the same rows: their per-degree GEMMs go out side by side in one launch
        ms, md = ops.irreps_linear_pair(node_input, self.merge_src.tp.weight, self.merge_src._bias(), self.merge_src.spec,
                                        self.merge_dst.tp.weight, self.merge_dst._bias(), self.merge_dst.spec)
        message = ops.gather_add(ms, md, g)
        if not self.nonlinear_message:
            value, alpha = self._linear_message(message, ectx)
        else:
            value, alpha = self._nonlinear_message(message, ectx)
        logit = ops.alpha_logits(alpha, self.alpha_dot, self.num_heads, self.mul_alpha_head,
                                 so3.C_SMOOTH_LEAKY_RELU_02)
        drop_p, seed = 0.0, 0
        if self.training and self.alpha_drop > 0.0:
            drop_p = self.alpha_drop
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        attn = ops.attn_aggregate(logit, value, g, self.num_heads, self.heads_layout, drop_p, seed)
        node_output = self.proj(attn)
        if self.proj_drop is not None:  # [ref: :524-525]
            node_output = self.proj_drop(node_output)
        return node_output

    def radial_module(self):
        """The RadialProfile evaluated on the shared radial basis (a member of the model's RadialBank)."""
        return self.sep_act.dtp_rad if self.nonlinear_message else self.sep.dtp_rad

    def _nonlinear_message(self, message, ectx):
        sa = self.sep_act
        table = sa.dtp.table
        M = ectx.coupling(table)
        weight = ectx.radial(sa.dtp_rad)
        if self.use_fused is True and self.act_sfc_spec.supported:
            value, alpha = ops.sep_fctp(message, M, weight, sa.flat_weight(), sa.lin._bias(), self.act_sfc_spec,
                                        weight2=self.sep_alpha.tp.weight, bias2=self.sep_alpha._bias())
        elif self.use_fused and sa.fused_spec is not None:
            value = ops.dtp_linear(message, M, weight, sa.lin.tp.weight, sa.lin._bias(), sa.fused_spec)
            alpha = ops.dtp_linear(message, M, weight, self.sep_alpha.tp.weight, self.sep_alpha._bias(),
                                   self.alpha_fused_spec)
        else:
            mid = ops.dtp(message, M, weight, table)
            alpha = self.sep_alpha(mid)
            value = sa.lin(mid)
        sv = self.sep_value
        gt = sa.gate
        if (self.use_fused is True and isinstance(gt, Gate) and sv.gate is None
                and ops.sep_fctp_gated_ok(sv.sfc_spec, value.shape[1], gt.S, gt.gated_layout, E=value.shape[0])):
            # the gate is folded into sep_value's kernels: its output rows are never written (csrc/sfcx.hip, *_gated)
            w2 = ectx.radial(sv.dtp_rad) if sv.dtp_rad is not None else None
            value = ops.sep_fctp_gated(value, ectx.coupling(sv.dtp.table), w2, sv.flat_weight(), sv.lin._bias(), sv.sfc_spec,
                                       (gt.S, gt.gated_layout, so3.C_SILU, so3.C_SIGMOID))
        else:
            value = sv(gt(value), ectx, use_fused=self.use_fused)
        return value, alpha

    def _linear_message(self, message, ectx):
        sep = self.sep
        table = sep.dtp.table
        M = ectx.coupling(table)
        weight = ectx.radial(sep.dtp_rad)
        W = sep.lin.tp.weight
        (l, _, K0, _, N0, off0) = sep.lin.spec.pairs[0]
        assert l == 0 and off0 == 0
        W0 = W[:K0 * N0].view(K0, N0)
        w_main = torch.cat([W0.index_select(1, self._idx_value).reshape(-1), W[K0 * N0:]])
        w_alpha = W0.index_select(1, self._idx_alpha).reshape(-1)
        b = sep.lin._bias()
        return ops.sep_fctp(message, M, weight, w_main, b.index_select(0, self._idx_value), self.lin_sfc_spec,
                            weight2=w_alpha, bias2=b.index_select(0, self._idx_alpha))


class DotProductAttention(nn.Module):
    """Scaled dot-product attention over irreps heads [ref: nets/dp_attention_transformer.py:68-160].  Queries: one
    LinearRS on the destination node; keys and values: ONE fused SeparableFCTP on the merged message producing 2H heads
    per edge (first H = keys), split by eqf_kv_split; logits with the ScaleFactor (:45-66) folded in by
    eqf_dp_logits_*; softmax + dropout + aggregation by the eqf_attn_aggregate_* kernels GraphAttention uses."""

    def __init__(self, irreps_node_input, irreps_node_attr, irreps_edge_attr, irreps_node_output, fc_neurons,
                 irreps_head, num_heads, irreps_pre_attn=None, rescale_degree=False, alpha_drop=0.1, proj_drop=0.1):
        super().__init__()
        self.irreps_node_input = Irreps(irreps_node_input)
        self.irreps_node_attr = Irreps(irreps_node_attr)
        self.irreps_edge_attr = Irreps(irreps_edge_attr)
        self.irreps_node_output = Irreps(irreps_node_output)
        self.irreps_pre_attn = self.irreps_node_input if irreps_pre_attn is None else Irreps(irreps_pre_attn)
        self.irreps_head = Irreps(irreps_head)
        self.num_heads = num_heads
        self.rescale_degree = rescale_degree
        if rescale_degree:
            raise NotImplementedError("rescale_degree=True is not used by any registered model")
        if [ir.l for _, ir in self.irreps_head] != sorted({ir.l for _, ir in self.irreps_head}):
            raise NotImplementedError("irreps_head must list each degree once, in ascending order")
        irreps_attn_heads = _simplified_sorted(self.irreps_head * num_heads)
        self.query = LinearRS(self.irreps_node_input, irreps_attn_heads)
        irreps_kv_heads = _simplified_sorted(self.irreps_head * num_heads * 2)
        self.merge_src = LinearRS(self.irreps_node_input, self.irreps_pre_attn, bias=True)
        self.merge_dst = LinearRS(self.irreps_node_input, self.irreps_pre_attn, bias=False)
        self.key_value = SeparableFCTP(self.irreps_pre_attn, self.irreps_edge_attr, irreps_kv_heads, fc_neurons,
                                       use_activation=False, norm_layer=None)
        self.heads_layout = RowLayout(irreps_attn_heads)
        self.alpha_drop = float(alpha_drop)
        self.alpha_dropout = nn.Dropout(alpha_drop) if alpha_drop != 0.0 else None  # marker module (no params)
        self.proj = LinearRS(irreps_attn_heads, self.irreps_node_output)
        # [ref: nets/dp_attention_transformer.py:116-119]
        self.proj_drop = EquivariantDropout(self.irreps_node_output, proj_drop) if proj_drop != 0.0 else None
        self.use_fused = True

    def radial_module(self):
        return self.key_value.dtp_rad

    def forward(self, node_input, node_attr=None, edge_src=None, edge_dst=None, edge_attr=None, edge_scalars=None,
                batch=None, ectx=None, **kwargs):
        g, H = ectx.graph, self.num_heads
        q = self.query(node_input)
        message = ops.gather_add(self.merge_src(node_input), self.merge_dst(node_input), g)
        kv = self.key_value(message, ectx, use_fused=self.use_fused)
        k, v = ops.kv_split(kv, H, self.heads_layout)
        logit = ops.dp_logits(q, k, g, H, self.heads_layout)
        drop_p, seed = 0.0, 0
        if self.training and self.alpha_drop > 0.0:
            drop_p = self.alpha_drop
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator: no device sync
        attn = ops.attn_aggregate(logit, v, g, H, self.heads_layout, drop_p, seed)
        node_output = self.proj(attn)
        if self.proj_drop is not None:  # [ref: nets/dp_attention_transformer.py:156-157]
            node_output = self.proj_drop(node_output)
        return node_output

    def extra_repr(self):
        return "rescale_degree={}".format(self.rescale_degree)


class FeedForwardNetwork(nn.Module):
    def __init__(self, irreps_node_input, irreps_node_attr, irreps_node_output, irreps_mlp_mid=None, proj_drop=0.1):
        super().__init__()
        self.irreps_node_input = Irreps(irreps_node_input)
        self.irreps_node_attr = Irreps(irreps_node_attr)
        self.irreps_mlp_mid = Irreps(irreps_mlp_mid) if irreps_mlp_mid is not None else self.irreps_node_input
        self.irreps_node_output = Irreps(irreps_node_output)
        self.fctp_1 = FullyConnectedTensorProductRescaleSwishGate(self.irreps_node_input, self.irreps_node_attr,
                                                                  self.irreps_mlp_mid, bias=True, rescale=_RESCALE)
        self.fctp_2 = FullyConnectedTensorProductRescale(self.irreps_mlp_mid, self.irreps_node_attr,
                                                         self.irreps_node_output, bias=True, rescale=_RESCALE)
        # [ref: :560-563]
        self.proj_drop = EquivariantDropout(self.irreps_node_output, proj_drop) if proj_drop != 0.0 else None

    def forward(self, node_input, node_attr=None, **kwargs):
        node_output = self.fctp_2(self.fctp_1(node_input, node_attr), node_attr)
        if self.proj_drop is not None:  # [ref: :569-570]
            node_output = self.proj_drop(node_output)
        return node_output


class GraphDropPath(nn.Module):
    """Per-graph stochastic depth [ref: nets/drop.py:45-61]: in training every graph of the batch keeps the branch with
    probability 1 - drop_prob (scaled by 1/keep), decided by one draw per graph from torch's CPU generator (fp64, the
    stream the fp64 oracle consumes under the same seed); the row scaling itself is eqf_segment_scale.  Inside a
    `droppath.device_draws` scope the draw happens in the kernel instead (eqf_segment_droppath: a function of the scope's
    seed, its call counter and the graph's index), which is what a captured step needs for a fresh mask per replay."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x, graph):
        if not self.drop_prob or not self.training:
            return x
        draws = droppath.active()
        if draws is not None:
            return droppath.segment_droppath(x, graph.batch, self.drop_prob, draws.seed, draws.next_call(), draws.word)
        keep = 1.0 - self.drop_prob
        r = torch.rand((graph.num_graphs, 1), dtype=torch.float64)
        s = ((keep + r).floor_() / keep).to(torch.float32).view(-1)
        return ops.segment_scale(x, s.to(x.device, non_blocking=True), graph.batch)

    def extra_repr(self):
        return "drop_prob={}".format(self.drop_prob)


class TransBlock(nn.Module):
    def __init__(self, irreps_node_input, irreps_node_attr, irreps_edge_attr, irreps_node_output, fc_neurons,
                 irreps_head, num_heads, irreps_pre_attn=None, rescale_degree=False, nonlinear_message=False,
                 alpha_drop=0.1, proj_drop=0.1, drop_path_rate=0.0, irreps_mlp_mid=None, norm_layer="layer"):
        super().__init__()
        self.irreps_node_input = Irreps(irreps_node_input)
        self.irreps_node_attr = Irreps(irreps_node_attr)
        self.irreps_edge_attr = Irreps(irreps_edge_attr)
        self.irreps_node_output = Irreps(irreps_node_output)
        self.irreps_mlp_mid = Irreps(irreps_mlp_mid) if irreps_mlp_mid is not None else self.irreps_node_input
        norm = get_norm_layer(norm_layer)
        self.norm_1 = norm(self.irreps_node_input)
        setattr(self, self.attn_name, self._make_attention(fc_neurons, irreps_head, num_heads, irreps_pre_attn,
                                                           rescale_degree, nonlinear_message, alpha_drop, proj_drop))
        self.drop_path = GraphDropPath(drop_path_rate) if drop_path_rate > 0.0 else None
        self.norm_2 = norm(self.irreps_node_input)
        self.ffn = FeedForwardNetwork(self.irreps_node_input, self.irreps_node_attr, self.irreps_node_output,
                                      self.irreps_mlp_mid, proj_drop)
        self.ffn_shortcut = None
        if self.irreps_node_input != self.irreps_node_output:
            self.ffn_shortcut = FullyConnectedTensorProductRescale(self.irreps_node_input, self.irreps_node_attr,
                                                                   self.irreps_node_output, bias=True,
                                                                   rescale=_RESCALE)

    attn_name = "ga"  # the attribute (= state_dict prefix) the attention module lives under

    def _make_attention(self, fc_neurons, irreps_head, num_heads, irreps_pre_attn, rescale_degree, nonlinear_message,
                        alpha_drop, proj_drop):
        return GraphAttention(self.irreps_node_input, self.irreps_node_attr, self.irreps_edge_attr,
                              self.irreps_node_input, fc_neurons, irreps_head, num_heads, irreps_pre_attn,
                              rescale_degree, nonlinear_message, alpha_drop, proj_drop)

    @property
    def attention(self):
        return getattr(self, self.attn_name)

    def _drop(self, x, ectx):
        return x if self.drop_path is None else self.drop_path(x, ectx.graph)

    def forward(self, node_input, node_attr=None, ectx=None, **kwargs):
        graph = ectx.graph
        node_output = node_input + self._drop(self.attention(self.norm_1(node_input, graph=graph), ectx=ectx), ectx)
        node_features = self._drop(self.ffn(self.norm_2(node_output, graph=graph), node_attr), ectx)
        if self.ffn_shortcut is not None:
            node_output = self.ffn_shortcut(node_output, node_attr)
        return node_output + node_features

    def forward_pair(self, a, b, node_attr=None, ectx=None):
        """The same block on a lazily summed input node_input = a + b, returning its output as a lazy pair as well
        (node_output, node_features): every residual add then rides on the layer norm that follows it (norm_1 here,
        norm_2, and the next block's norm_1 or the model's final norm) instead of being its own launch."""
        node_input, h = self.norm_1.forward_sum(a, b, graph=ectx.graph)
        node_output, h2 = self.norm_2.forward_sum(node_input, self._drop(self.attention(h, ectx=ectx), ectx),
                                                  graph=ectx.graph)
        node_features = self._drop(self.ffn(h2, node_attr), ectx)
        if self.ffn_shortcut is not None:
            node_output = self.ffn_shortcut(node_output, node_attr)
        return node_output, node_features


class DPTransBlock(TransBlock):
    """[ref: nets/dp_attention_transformer.py:163-252] the pre-norm block with DotProductAttention under `dpa`."""
    attn_name = "dpa"

    def _make_attention(self, fc_neurons, irreps_head, num_heads, irreps_pre_attn, rescale_degree, nonlinear_message,
                        alpha_drop, proj_drop):
        return DotProductAttention(self.irreps_node_input, self.irreps_node_attr, self.irreps_edge_attr,
                                   self.irreps_node_input, fc_neurons, irreps_head, num_heads, irreps_pre_attn,
                                   rescale_degree, alpha_drop, proj_drop)


class NodeEmbeddingNetwork(nn.Module):
    def __init__(self, irreps_node_embedding, max_atom_type, bias=True):
        super().__init__()
        self.max_atom_type = max_atom_type
        self.irreps_node_embedding = Irreps(irreps_node_embedding)
        self.atom_type_lin = LinearRS(Irreps("{}x0e".format(max_atom_type)), self.irreps_node_embedding, bias=bias)
        self.atom_type_lin.tp.weight.data.mul_(max_atom_type ** 0.5)
        self.D = self.atom_type_lin.layout_out.dim
        self.C = self.atom_type_lin.layout_out.mul_of(0)

    def forward(self, node_atom):
        """one_hot(node_atom) @ W + b == row lookup; returns the embedding only (attr/one-hot are unused)."""
        W = self.atom_type_lin.tp.weight.view(self.max_atom_type, self.C)
        emb = ops.embed(node_atom.to(torch.int32), W, self.atom_type_lin._bias(), self.D)
        return emb, None, None


class ScaledScatter(nn.Module):
    def __init__(self, avg_aggregate_num):
        super().__init__()
        self.avg_aggregate_num = avg_aggregate_num + 0.0

    def forward(self, x, ptr, seg_of, nseg):
        return ops.segment_sum(x, ptr, seg_of, nseg, 1.0 / (self.avg_aggregate_num ** 0.5))

    def extra_repr(self):
        return "avg_aggregate_num={}".format(self.avg_aggregate_num)


class EdgeDegreeEmbeddingNetwork(nn.Module):
    def __init__(self, irreps_node_embedding, irreps_edge_attr, fc_neurons, avg_aggregate_num):
        super().__init__()
        irreps_node_embedding = Irreps(irreps_node_embedding)
        self.exp = LinearRS(Irreps("1x0e"), irreps_node_embedding, bias=_USE_BIAS, rescale=_RESCALE)
        self.dw = DepthwiseTensorProduct(irreps_node_embedding, irreps_edge_attr, irreps_node_embedding,
                                         internal_weights=False, bias=False)
        self.rad = RadialProfile(fc_neurons + [self.dw.tp.weight_numel])
        self.proj = LinearRS(self.dw.table.irreps_out, irreps_node_embedding)
        self.scale_scatter = ScaledScatter(avg_aggregate_num)
        self.fused_spec = ops.DtpLinearSpec.make(self.dw.table, self.proj.layout_out)
        self.sfc_spec = ops.SfcSpec(self.dw.table, self.proj.layout_out)
        self.D = self.exp.layout_out.dim
        self.C = self.exp.layout_out.mul_of(0)
        self.use_fused = True
        self.collapsed_spec = ops.EdgeDegSpec(self.dw.table, self.proj.spec, self.rad.net[-1].weight.shape[1])

    # src_features is exp(ones): the same row for every edge, zeros outside the C channels of 0e.  Only the l1 == 0 paths of the
    # table see anything else; radial last layer, depth-wise product and projection fold into one [sum N_l, 64] matrix and the
    # operator becomes one E x 64 GEMM and a segmented scatter (csrc/edgedeg.hip).  EQF_EDGE_DEGREE_COLLAPSED=0 keeps the fused
    # SeparableFCTP (A/B measurements of one build).
    use_collapsed = os.environ.get("EQF_EDGE_DEGREE_COLLAPSED", "1") == "1"

    def collapses(self, edge_sh):
        """The collapsed path applies: fused kernels asked for, an SE(3) table, and nothing differentiates through the
        spherical harmonics (force training keeps the fused operator, also at second order)."""
        return bool(self.use_collapsed and self.use_fused is True and self.sfc_spec.supported and self.collapsed_spec.supported
                    and self.collapsed_spec.C == self.C and not edge_sh.requires_grad)

    def forward(self, node_input, ectx):
        g = ectx.graph
        if self.collapses(ectx.edge_sh) and ectx.wants_hidden(self.rad):
            spec = self.collapsed_spec
            At, a = ops.edgedeg_fold(self.rad.net[-1].weight, self.rad.offset, self.exp.tp.weight, self.exp._bias(),
                                     self.proj.tp.weight, spec)
            z = ops.dense_linear(ectx.radial_hidden(self.rad), At, a)
            return ops.edgedeg_scatter(z, ectx.coupling(self.dw.table), self.proj._bias(), g, spec,
                                       1.0 / (self.scale_scatter.avg_aggregate_num ** 0.5))
        # exp(ones): the same row for every node == lookup of row 0
        zeros = torch.zeros(g.N, dtype=torch.int32, device=node_input.device)
        node_features = ops.embed(zeros, self.exp.tp.weight.view(1, self.C), self.exp._bias(), self.D)
        weight = ectx.radial(self.rad)
        src_features = ops.gather_add(node_features, None, g)
        M = ectx.coupling(self.dw.table)
        if self.use_fused is True and self.sfc_spec.supported:
            edge_features = ops.sep_fctp(src_features, M, weight, self.proj.tp.weight, self.proj._bias(), self.sfc_spec)
        elif self.use_fused and self.fused_spec is not None:
            edge_features = ops.dtp_linear(src_features, M, weight, self.proj.tp.weight, self.proj._bias(),
                                           self.fused_spec)
        else:
            edge_features = self.proj(ops.dtp(src_features, M, weight, self.dw.table))
        seg_of = g.dst
        return self.scale_scatter(edge_features, g.row_ptr, seg_of, g.N)
