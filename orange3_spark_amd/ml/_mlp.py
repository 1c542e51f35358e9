"""MultilayerPerceptronClassifier (``pyspark.ml.classification``).

Reached through the Classification widget's reflection.  Network: affine
layers with sigmoid activations and a softmax output, cross-entropy loss averaged over
the (weighted) rows, trained with L-BFGS (default) or gradient descent.

MI355X mapping: on a GPU session whose features column is a plain resident vector column
(bf16 or fp32) a network with one hidden layer (``layers = [d, H, K]``, d <= 256, H <= 128,
K <= 32 and few enough 32 x 32 blocks of W1, ``ops.mlp.gate_reason``) takes every optimiser
evaluation from one launch of the fused MLP pass over the stored rows, and ``transform`` takes
its logits from the forward half of that kernel (``ops/mlp.py``, ``csrc/mlp.hip``): no fp32
copy of the table and no per-chunk temporaries.  ``O3S_MLP_KERNEL=0``, deeper or wider
networks, CPU sessions and sparse, lineage and spilled columns run the torch program instead:
forward + backward over the rank's rows as chunked fp32 GEMMs (hipBLASLt) under autograd.
Either way ONE flat gradient vector is all-reduced per evaluation (models/dist_opt.py) -- data
parallelism over row shards, like Spark's treeAggregate.
The flat weight layout is Spark's (per layer: the [in, out] weight block stored
column-major as an out x in matrix, then the bias), so saved ``weights`` interoperate.
"""
from __future__ import annotations

import numpy as np
import torch

from ..models import dist_opt
from ..ops import linear_predict as LP
from ..ops import mlp as MLP
from . import common as U
from .base import Estimator, Model
from .linalg import DenseVector
from .param import (HasBlockSize, HasFeaturesCol, HasLabelCol, HasMaxIter, HasPredictionCol, HasProbabilityCol,
                    HasRawPredictionCol, HasSeed, HasSolver, HasStepSize, HasThresholds, HasTol, TypeConverters,
                    keyword_only, shared)
from .util import MLReadable, MLWritable, apply_metadata, read_data, register, vec_col, write_data


class _MLPParams(HasFeaturesCol, HasLabelCol, HasPredictionCol, HasProbabilityCol, HasRawPredictionCol,
                 HasMaxIter, HasTol, HasSeed, HasStepSize, HasSolver, HasBlockSize, HasThresholds):
    layers = shared("layers", "Sizes of layers from input layer to output layer E.g., Array(780, 100, 10) means "
                              "780 inputs, one hidden layer with 100 neurons and output layer of 10 neurons.",
                    TypeConverters.toListInt)
    initialWeights = shared("initialWeights", "The initial weights of the model.", TypeConverters.toVector)

    def __init__(self):
        super().__init__()
        self._setDefault(maxIter=100, tol=1e-6, blockSize=128, stepSize=0.03, solver="l-bfgs", seed=0)


def layer_slices(layers):
    """[(w_offset, b_offset, n_in, n_out)] of the flat Spark weight vector."""
    out, off = [], 0
    for i, o in zip(layers[:-1], layers[1:]):
        out.append((off, off + i * o, i, o))
        off += i * o + o
    return out, off


def forward(theta: torch.Tensor, X: torch.Tensor, layers) -> torch.Tensor:
    """Logits of the output layer (pre-softmax), theta in Spark's flat layout."""
    h = X
    sl, _ = layer_slices(layers)
    for li, (wo, bo, i, o) in enumerate(sl):
        W = theta[wo:wo + i * o].reshape(i, o)       # out x in column-major == [in, out] row-major
        h = h @ W + theta[bo:bo + o]
        if li < len(sl) - 1:
            h = torch.sigmoid(h)
    return h


def init_weights(layers, seed: int) -> np.ndarray:
    """Uniform(-r, r), r = sqrt(6 / (in + out)) per layer, zero biases (Glorot)."""
    sl, total = layer_slices(layers)
    rng = np.random.default_rng(seed)
    x = np.zeros(total)
    for wo, bo, i, o in sl:
        r = np.sqrt(6.0 / (i + o))
        x[wo:wo + i * o] = rng.uniform(-r, r, i * o)
    return x


class _FusedMLPObjective(dist_opt.Objective):
    """The objective of a ``[d, H, K]`` network with the loss and gradient of a row range from
    one fused pass (``ops.mlp.mlp_pass``) over the stored rows, in place of autograd over
    ``forward``.

    ``local`` returns what ``Objective.local`` returns for ``local_loss`` of ``_fit``: the loss
    sum and the flat fp64 gradient in Spark's layout.  The full batch is one launch, a subset of
    ``parts`` one launch per chunk.  ``pass_fn`` replaces the kernel wrapper (tests run the
    objective on the CPU with ``ops.mlp.mlp_pass_torch``)."""

    def __init__(self, comm, device, X, y, layers, W: float, chunk: int = 1 << 18, pass_fn=None):
        super().__init__(comm, device, X.shape[0], None, W, chunk=chunk)
        if len(layers) != 3:
            raise ValueError("the fused MLP objective takes one hidden layer")
        self.X, self.y, self.layers = X, y, [int(v) for v in layers]
        self.pass_fn = pass_fn
        self.n = int(X.shape[0])

    def local(self, theta, parts=None):
        fn = self.pass_fn or MLP.mlp_pass
        (sl1, sl2), total_len = layer_slices(self.layers)
        th = theta.detach()
        W1, b1 = th[sl1[0]:sl1[1]].reshape(sl1[2], sl1[3]), th[sl1[1]:sl1[1] + sl1[3]]
        W2, b2 = th[sl2[0]:sl2[1]].reshape(sl2[2], sl2[3]), th[sl2[1]:sl2[1] + sl2[3]]
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        grad = torch.zeros(total_len, dtype=torch.float64, device=self.device)
        if parts is None or parts is self.parts:
            parts = [(0, self.n)]                      # the full batch: one launch
        for a, b in parts:
            if b <= a:
                continue
            gW1, gb1, gW2, gb2, l = fn(self.X[a:b], self.y[a:b], W1, b1, W2, b2)
            grad += torch.cat([gW1.reshape(-1), gb1, gW2.reshape(-1), gb2]).to(torch.float64)
            total += l.to(torch.float64)
        return total, grad


def _kernel_rows(df, name: str, H: int, K: int):
    """The stored rows ``[n, d]`` of the features column if the fused MLP passes take them -- a
    plain resident vector column (not lineage, spilled or sparse) that ``mlp_kernel_ok``
    accepts, with the kernels enabled -- else None."""
    if not MLP.mlp_enabled():
        return None
    col = df.column_data(name)
    d = getattr(col, "size", 0)
    if not 1 <= d <= MLP.MAX_D:
        return None
    rows = LP.column_rows(col, d)
    if rows is None:
        return None
    X = rows if d == rows.shape[1] else rows[:, :d]
    return X if MLP.mlp_kernel_ok(X, H, K) else None


class _KernelRows:
    """The stored rows of a features column on their way to ``_raw`` (``mlp_logits``)."""

    def __init__(self, X: torch.Tensor):
        self.X = X


@register("org.apache.spark.ml.classification.MultilayerPerceptronClassifier")
class MultilayerPerceptronClassifier(Estimator, _MLPParams, MLWritable, MLReadable):
    """Classifier trainer based on the Multilayer Perceptron. Each layer has sigmoid
    activation function, output layer has softmax. Number of inputs has to be equal to the
    size of feature vectors. Number of outputs has to be equal to the total number of labels.
    """

    @keyword_only
    def __init__(self, *, featuresCol="features", labelCol="label", predictionCol="prediction", maxIter=100,
                 tol=1e-6, seed=None, layers=None, blockSize=128, stepSize=0.03, solver="l-bfgs",
                 initialWeights=None, probabilityCol="probability", rawPredictionCol="rawPrediction"):
        super().__init__()
        self._set(**self._input_kwargs)

    @keyword_only
    def setParams(self, *, featuresCol="features", labelCol="label", predictionCol="prediction", maxIter=100,
                  tol=1e-6, seed=None, layers=None, blockSize=128, stepSize=0.03, solver="l-bfgs",
                  initialWeights=None, probabilityCol="probability", rawPredictionCol="rawPrediction"):
        return self._set(**self._input_kwargs)

    def _fit(self, df):
        g = self.getOrDefault
        comm = df.comm
        sizes = [int(v) for v in g(self.layers)] if self.isDefined(self.layers) and g(self.layers) else []
        X = _kernel_rows(df, g(self.featuresCol), sizes[1], sizes[2]) if len(sizes) == 3 else None
        # every fused rank has the input layer's width, so the ranks agree on d
        fused = X is not None and X.shape[1] == sizes[0]
        if not fused:
            X = U.dense_features(df, g(self.featuresCol))
        y = U.numeric_column(df, g(self.labelCol))
        if not self.isDefined(self.layers) or not g(self.layers):
            raise ValueError("MultilayerPerceptronClassifier requires the layers param")
        layers = [int(v) for v in g(self.layers)]
        if X.shape[1] != layers[0] and X.shape[0]:
            raise ValueError(f"Dimensions mismatch: features {X.shape[1]} vs input layer {layers[0]}")
        K = layers[-1]
        dev = X.device
        dt = dist_opt.compute_dtype(dev)
        yl = y.to(dev).long()
        if yl.numel() and int(comm.max_scalar(float(yl.max()))) >= K:
            raise ValueError(f"labels must be in [0, {K}) for an output layer of size {K}")
        n = X.shape[0]
        W = float(comm.sum_scalar(n))

        def local_loss(theta, a, b):
            logits = forward(theta, X[a:b].to(dt), layers)
            return torch.nn.functional.cross_entropy(logits, yl[a:b], reduction="sum")

        if fused:
            obj = _FusedMLPObjective(comm, dev, X, yl.to(torch.int32), layers, W, chunk=1 << 18)
        else:
            obj = dist_opt.Objective(comm, dev, n, local_loss, W, chunk=1 << 18)
        if self.isDefined(self.initialWeights) and g(self.initialWeights) is not None:
            x0 = np.asarray(g(self.initialWeights).toArray(), dtype=np.float64)
        else:
            x0 = init_weights(layers, int(g(self.seed)) & 0xFFFFFFFF)
        if g(self.solver) == "gd":
            res = dist_opt.gradient_descent(obj, x0, g(self.maxIter), g(self.stepSize), g(self.tol))
        else:
            res = dist_opt.lbfgs(obj, x0, g(self.maxIter), g(self.tol))
        m = MultilayerPerceptronClassificationModel._from(layers, res.x)
        m.summary = _TrainingSummary(res.history, res.iterations)
        return m._with_parent(self)


class _TrainingSummary:
    def __init__(self, history, iterations):
        self.objectiveHistory = list(history)
        self.totalIterations = int(iterations)


@register("org.apache.spark.ml.classification.MultilayerPerceptronClassificationModel")
class MultilayerPerceptronClassificationModel(U.ProbabilisticClassifierMixin, Model, _MLPParams, MLWritable,
                                              MLReadable):
    """Model fitted by MultilayerPerceptronClassifier."""

    def evaluate(self, df):
        """Multiclass metrics of this model's predictions on ``df`` (Spark >= 3.1)."""
        from . import _summary as S
        g = self.getOrDefault
        return S.ClassificationSummary(lambda: self.transform(df), labelCol=g(self.labelCol),
                                       predictionCol=g(self.predictionCol))

    def __init__(self):
        super().__init__()
        self._layers = []
        self._w = np.zeros(0)
        self.summary = None

    @classmethod
    def _from(cls, layers, weights):
        m = cls()
        m._layers = [int(v) for v in layers]
        m._w = np.asarray(weights, dtype=np.float64)
        m._set(layers=m._layers)
        return m

    @property
    def weights(self) -> DenseVector:
        return DenseVector(self._w)

    @property
    def numFeatures(self) -> int:
        return self._layers[0]

    @property
    def numClasses(self) -> int:
        return self._layers[-1]

    def _features_for_predict(self, df, name):
        """Operand of ``_raw`` for a transform: the stored rows when the logits kernel takes
        them (:func:`_kernel_rows`) and the width matches, else the dense features."""
        if len(self._layers) == 3:
            X = _kernel_rows(df, name, self._layers[1], self._layers[2])
            if X is not None and X.shape[1] == self._layers[0]:
                return _KernelRows(X)
        return U.dense_features(df, name)

    def _packed(self, device):
        """The kernel operands of the weights on ``device``, built at the first use and kept
        for as long as the weights are the same array."""
        cache = self.__dict__.get("_mlp_cache")
        if cache is None or cache[0] is not self._w or cache[1] != device:
            (sl1, sl2), _ = layer_slices(self._layers)
            th = torch.from_numpy(self._w)
            W1, b1 = th[sl1[0]:sl1[1]].reshape(sl1[2], sl1[3]), th[sl1[1]:sl1[1] + sl1[3]]
            W2, b2 = th[sl2[0]:sl2[1]].reshape(sl2[2], sl2[3]), th[sl2[1]:sl2[1] + sl2[3]]
            cache = self.__dict__["_mlp_cache"] = (self._w, device, MLP.pack(W1, b1, W2, b2, device=device))
        return cache[2]

    def __getstate__(self):
        st = dict(self.__dict__)
        st.pop("_mlp_cache", None)
        return st

    def _raw(self, X):
        if isinstance(X, _KernelRows):
            return MLP.mlp_logits(X.X, None, None, None, None, packed=self._packed(X.X.device)).to(torch.float64)
        dt = dist_opt.compute_dtype(X.device)
        theta = torch.from_numpy(self._w).to(X.device, dt)
        return forward(theta, X.to(dt)[:, : self.numFeatures], self._layers).to(torch.float64)

    def _save_data(self, path):
        write_data(path, {"weights": vec_col([self.weights])})

    @classmethod
    def _load_impl(cls, path, meta):
        from .util import vector_from_struct
        t = read_data(path).to_pylist()[0]
        layers = meta.get("paramMap", {}).get("layers")
        m = cls._from(layers, vector_from_struct(t["weights"]).toArray())
        apply_metadata(m, meta)
        return m
