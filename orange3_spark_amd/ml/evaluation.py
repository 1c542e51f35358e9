"""Evaluators (``pyspark.ml.evaluation`` surface).

The Evaluation widget reflects over this module and parses the supported metric names
from the ``metricName`` doc string with ``doc.split('(')[-1].replace(')','').split('|')``
(orangecontrib/spark/widgets/ml/spark_ml_evaluation.py:43), so every ``metricName``
doc ends in ``(a|b|c)``.

Distributed strategy: per-rank sufficient statistics (confusion matrix, error sums,
score histograms) are combined with one all-reduce; exact ROC/PR sorting gathers
(score, label, weight) only when the global row count is small enough.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..frame import column as C
from .base import Evaluator
from .param import (HasFeaturesCol, HasLabelCol, HasPredictionCol, HasProbabilityCol, HasRawPredictionCol,
                    HasWeightCol, TypeConverters, add_accessors, keyword_only, shared)
from .util import MLReadable, MLWritable, register

EXACT_AUC_MAX_ROWS = 1 << 24
HIST_BINS = 1 << 20


def _num(df, name, dtype=torch.float64):
    """Column tensor; ``dtype=None`` keeps the stored dtype (the kernels convert in registers)."""
    c = df.column_data(name)
    if isinstance(c, (C.NumericColumn, C.VectorColumn)):
        return c.data if dtype is None else c.data.to(dtype)
    raise TypeError(f"column {name} is not numeric")


def _weights(df, ev, n, device, required=True):
    """Weight column, or unit weights (``None`` when not ``required``: kernels skip the read)."""
    if ev.isDefined(ev.weightCol) and ev.getOrDefault(ev.weightCol):
        return _num(df, ev.getOrDefault(ev.weightCol)).to(device)
    return torch.ones(n, dtype=torch.float64, device=device) if required else None


def _exact_curve(score: np.ndarray, label: np.ndarray, w: np.ndarray):
    """(thresholds desc, cum TP, cum FP, P, N) at every distinct score (Spark
    BinaryClassificationMetrics without down-sampling)."""
    order = np.argsort(-score, kind="stable")
    s, l, w = score[order], label[order], w[order]
    pos_w = w * (l > 0.5)
    neg_w = w * (l <= 0.5)
    bounds = np.nonzero(np.diff(s))[0]
    ends = np.concatenate([bounds, [len(s) - 1]]).astype(np.int64) if len(s) else np.array([], dtype=np.int64)
    tp = np.cumsum(pos_w)[ends] if len(s) else np.array([])
    fp = np.cumsum(neg_w)[ends] if len(s) else np.array([])
    return s[ends] if len(s) else np.array([]), tp, fp, pos_w.sum(), neg_w.sum()


def _exact_curve_device(s: torch.Tensor, y: torch.Tensor, w: torch.Tensor):
    """:func:`_exact_curve` on the device (stable radix sort, cumulative sums, distinct-score
    boundaries) -- only the curve points cross to the host."""
    if not s.numel():
        z = np.array([])
        return z, z, z, 0.0, 0.0
    order = torch.sort(-s, stable=True).indices
    ss, yy, ww = s[order], y[order], w[order]
    pos_w = ww * (yy > 0.5)
    neg_w = ww * (yy <= 0.5)
    ends = torch.cat([torch.nonzero(ss[1:] != ss[:-1]).flatten(),
                      torch.tensor([ss.numel() - 1], device=ss.device)])
    tp = torch.cumsum(pos_w, 0)[ends]
    fp = torch.cumsum(neg_w, 0)[ends]
    return (ss[ends].cpu().numpy(), tp.cpu().numpy(), fp.cpu().numpy(), float(pos_w.sum()), float(neg_w.sum()))


def _hist_curve(comm, score: torch.Tensor, label: torch.Tensor, w):
    """Large-data path: 2^20-bin score histograms per class (one fused pass, ops/evaluation.py
    score_hist kernel on the GPU), one all-reduce (16 MB fp64).  Thresholds are bin edges."""
    from ..ops import evaluation as EV
    if score.numel():
        mn, mx = torch.aminmax(score)
        lohi = torch.tensor([float(mn), -float(mx)], dtype=torch.float64, device=comm.device)
    else:
        lohi = torch.tensor([math.inf, math.inf], dtype=torch.float64, device=comm.device)
    comm.all_reduce(lohi, "min")
    lo, hi = float(lohi[0]), -float(lohi[1])
    span = max(hi - lo, 1e-12)
    h = EV.score_hist(score, label, lo, span, HIST_BINS, w)
    comm.all_reduce(h)
    hp, hn = h[0].flip(0).cpu().numpy(), h[1].flip(0).cpu().numpy()
    keep = (hp + hn) > 0
    edges = lo + (np.arange(HIST_BINS, dtype=np.float64)[::-1]) * (span / (HIST_BINS - 1))
    return edges[keep], np.cumsum(hp)[keep], np.cumsum(hn)[keep], hp.sum(), hn.sum()


def binary_curve(comm, score: torch.Tensor, label: torch.Tensor, w):
    """Global (thresholds, tp, fp, P, N): exact when the row count is small, else histogram."""
    n = comm.sum_scalar(int(score.shape[0]))
    if n <= EXACT_AUC_MAX_ROWS:
        if w is None:
            w = torch.ones(score.shape[0], dtype=torch.float64, device=score.device)
        s, y, ww = (comm.all_gather_v(t.to(torch.float64).contiguous()) for t in (score, label, w))
        if s.is_cuda:
            return _exact_curve_device(s, y, ww)
        return _exact_curve(s.cpu().numpy(), y.cpu().numpy(), ww.cpu().numpy())
    return _hist_curve(comm, score, label, w)


def curve_areas(tp, fp, P, N):
    """(areaUnderROC, areaUnderPR) by the trapezoid rule over the curve points."""
    tpr = np.concatenate([[0.0], tp / P if P > 0 else np.zeros_like(tp), [1.0]])
    fpr = np.concatenate([[0.0], fp / N if N > 0 else np.zeros_like(fp), [1.0]])
    roc = float(np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) / 2))
    if not len(tp):
        return roc, 0.0
    recall = tp / P if P > 0 else np.zeros_like(tp)
    precision = np.where(tp + fp > 0, tp / np.maximum(tp + fp, 1e-300), 1.0)
    rec = np.concatenate([[0.0], recall])
    prec = np.concatenate([[precision[0]], precision])
    return roc, float(np.sum((rec[1:] - rec[:-1]) * (prec[1:] + prec[:-1]) / 2))


@add_accessors
@register("org.apache.spark.ml.evaluation.BinaryClassificationEvaluator")
class BinaryClassificationEvaluator(Evaluator, HasLabelCol, HasRawPredictionCol, HasWeightCol, MLWritable,
                                    MLReadable):
    """Evaluator for binary classification: expects rawPrediction (vector or double score)
    and label columns."""

    metricName = shared("metricName", "metric name in evaluation (areaUnderROC|areaUnderPR)",
                        TypeConverters.toString)
    numBins = shared("numBins", "Number of bins to down-sample the curves (ROC curve, PR curve) in area "
                                "computation. If 0, no down-sampling will occur. Must be >= 0.", TypeConverters.toInt)

    @keyword_only
    def __init__(self, *, rawPredictionCol="rawPrediction", labelCol="label", metricName="areaUnderROC",
                 weightCol=None, numBins=1000):
        super().__init__()
        self._setDefault(metricName="areaUnderROC", numBins=1000, rawPredictionCol="rawPrediction", labelCol="label")
        self._set(**self._input_kwargs)

    @keyword_only
    def setParams(self, *, rawPredictionCol="rawPrediction", labelCol="label", metricName="areaUnderROC",
                  weightCol=None, numBins=1000):
        return self._set(**self._input_kwargs)

    def _scores(self, df):
        """(score view, label, weight or None) in their stored dtypes -- no copies."""
        raw = df.column_data(self.getOrDefault(self.rawPredictionCol))
        if isinstance(raw, C.VectorColumn):
            s = raw.data[:, 1] if raw.data.shape[1] > 1 else raw.data[:, 0]
        else:
            s = raw.data
        y = _num(df, self.getOrDefault(self.labelCol), None).to(s.device)
        w = _weights(df, self, s.shape[0], s.device, required=False)
        return s, y, w

    def _evaluate(self, df):
        s, y, w = self._scores(df)
        _, tp, fp, P, N = binary_curve(df.comm, s, y, w)
        roc, pr = curve_areas(tp, fp, P, N)
        return roc if self.getOrDefault(self.metricName) == "areaUnderROC" else pr

    def isLargerBetter(self):
        return True


_MC_METRICS = ("f1|accuracy|weightedPrecision|weightedRecall|weightedTruePositiveRate|weightedFalsePositiveRate|"
               "weightedFMeasure|truePositiveRateByLabel|falsePositiveRateByLabel|precisionByLabel|recallByLabel|"
               "fMeasureByLabel|logLoss|hammingLoss")


@add_accessors
@register("org.apache.spark.ml.evaluation.MulticlassClassificationEvaluator")
class MulticlassClassificationEvaluator(Evaluator, HasLabelCol, HasPredictionCol, HasWeightCol, HasProbabilityCol,
                                        MLWritable, MLReadable):
    """Evaluator for multiclass classification (confusion matrix all-reduced over ranks)."""

    metricName = shared("metricName", f"metric name in evaluation ({_MC_METRICS})", TypeConverters.toString)
    metricLabel = shared("metricLabel", "The class whose metric will be computed in truePositiveRateByLabel|"
                                        "falsePositiveRateByLabel|precisionByLabel|recallByLabel|fMeasureByLabel."
                                        " Must be >= 0. The default value is 0.", TypeConverters.toFloat)
    beta = shared("beta", "The beta value used in weightedFMeasure|fMeasureByLabel. Must be > 0. "
                          "The default value is 1.", TypeConverters.toFloat)
    eps = shared("eps", "log-loss is undefined for p=0 or p=1, so probabilities are clipped to "
                        "max(eps, min(1 - eps, p)). Must be in range (0, 0.5). The default value is 1e-15.",
                 TypeConverters.toFloat)

    @keyword_only
    def __init__(self, *, predictionCol="prediction", labelCol="label", metricName="f1", weightCol=None,
                 metricLabel=0.0, probabilityCol="probability", beta=1.0, eps=1e-15):
        super().__init__()
        self._setDefault(metricName="f1", metricLabel=0.0, beta=1.0, eps=1e-15)
        self._set(**self._input_kwargs)

    @keyword_only
    def setParams(self, *, predictionCol="prediction", labelCol="label", metricName="f1", weightCol=None,
                  metricLabel=0.0, probabilityCol="probability", beta=1.0, eps=1e-15):
        return self._set(**self._input_kwargs)

    def _evaluate(self, df):
        g = self.getOrDefault
        comm = df.comm
        metric = g(self.metricName)
        y = _num(df, g(self.labelCol), None)
        if metric == "logLoss":
            w = _weights(df, self, y.shape[0], y.device)
            prob = df.column_data(g(self.probabilityCol)).data.to(torch.float64)
            p = prob.gather(1, y.long()[:, None]).squeeze(1).clamp(g(self.eps), 1 - g(self.eps))
            t = torch.stack([(-torch.log(p) * w).sum(), w.sum()])
            comm.all_reduce(t)
            return float(t[0] / t[1])
        from ..ops import evaluation as EV
        pred = _num(df, g(self.predictionCol), None).to(y.device)
        k = int(comm.max_scalar(float(max(y.max().item() if y.numel() else 0, pred.max().item() if pred.numel() else 0)))) + 1
        k = max(k, int(g(self.metricLabel)) + 1)
        cm = EV.confusion(y, pred, k, _weights(df, self, y.shape[0], y.device, required=False)).reshape(-1)
        comm.all_reduce(cm)
        cm = cm.reshape(k, k).cpu().numpy()       # rows = label, cols = prediction
        return _multiclass_metric(cm, metric, int(g(self.metricLabel)), g(self.beta))

    def isLargerBetter(self):
        return self.getOrDefault(self.metricName) not in ("weightedFalsePositiveRate", "falsePositiveRateByLabel",
                                                          "logLoss", "hammingLoss")


def _multiclass_metric(cm: np.ndarray, metric: str, label: int, beta: float) -> float:
    total = cm.sum()
    tp = np.diag(cm)
    lab_cnt = cm.sum(1)
    pred_cnt = cm.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = np.where(pred_cnt > 0, tp / pred_cnt, 0.0)
        recall = np.where(lab_cnt > 0, tp / lab_cnt, 0.0)
        fp = pred_cnt - tp
        neg = total - lab_cnt
        fpr = np.where(neg > 0, fp / neg, 0.0)
        b2 = beta * beta
        fm = np.where(precision + recall > 0, (1 + b2) * precision * recall / (b2 * precision + recall), 0.0)
    wts = lab_cnt / total if total else lab_cnt
    if metric == "accuracy":
        return float(tp.sum() / total) if total else 0.0
    if metric == "hammingLoss":
        return float(1 - tp.sum() / total) if total else 0.0
    if metric in ("weightedPrecision",):
        return float((precision * wts).sum())
    if metric in ("weightedRecall", "weightedTruePositiveRate"):
        return float((recall * wts).sum())
    if metric == "weightedFalsePositiveRate":
        return float((fpr * wts).sum())
    if metric in ("f1", "weightedFMeasure"):
        if metric == "f1":
            with np.errstate(divide="ignore", invalid="ignore"):
                f1 = np.where(precision + recall > 0, 2 * precision * recall / (precision + recall), 0.0)
            return float((f1 * wts).sum())
        return float((fm * wts).sum())
    if metric == "truePositiveRateByLabel" or metric == "recallByLabel":
        return float(recall[label]) if label < len(recall) else 0.0
    if metric == "falsePositiveRateByLabel":
        return float(fpr[label]) if label < len(fpr) else 0.0
    if metric == "precisionByLabel":
        return float(precision[label]) if label < len(precision) else 0.0
    if metric == "fMeasureByLabel":
        return float(fm[label]) if label < len(fm) else 0.0
    # Spark 1.x names
    if metric == "precision":
        return float(tp.sum() / total)
    if metric == "recall":
        return float(tp.sum() / total)
    raise ValueError(f"unsupported metric {metric}")


@add_accessors
@register("org.apache.spark.ml.evaluation.RegressionEvaluator")
class RegressionEvaluator(Evaluator, HasLabelCol, HasPredictionCol, HasWeightCol, MLWritable, MLReadable):
    """Evaluator for regression (sufficient statistics all-reduced in fp64)."""

    metricName = shared("metricName", "metric name in evaluation (rmse|mse|r2|mae|var)", TypeConverters.toString)
    throughOrigin = shared("throughOrigin", "whether the regression is through the origin.",
                           TypeConverters.toBoolean)

    @keyword_only
    def __init__(self, *, predictionCol="prediction", labelCol="label", metricName="rmse", weightCol=None,
                 throughOrigin=False):
        super().__init__()
        self._setDefault(metricName="rmse", throughOrigin=False)
        self._set(**self._input_kwargs)

    @keyword_only
    def setParams(self, *, predictionCol="prediction", labelCol="label", metricName="rmse", weightCol=None,
                  throughOrigin=False):
        return self._set(**self._input_kwargs)

    def _evaluate(self, df):
        g = self.getOrDefault
        from ..ops import evaluation as EV
        y = _num(df, g(self.labelCol), None)
        p = _num(df, g(self.predictionCol), None).to(y.device)
        st = EV.regression_stats(y, p, _weights(df, self, y.shape[0], y.device, required=False))
        df.comm.all_reduce(st)
        W, se, ae, sy, syy, sp, spp = st.tolist()
        mse = se / W
        m = g(self.metricName)
        if m == "mse":
            return mse
        if m == "rmse":
            return math.sqrt(mse)
        if m == "mae":
            return ae / W
        if m == "r2":
            ss_tot = syy if g(self.throughOrigin) else syy - sy * sy / W
            return 1 - se / ss_tot if ss_tot else float("nan")
        if m == "var":
            return spp / W - (sp / W) ** 2
        raise ValueError(m)

    def isLargerBetter(self):
        return self.getOrDefault(self.metricName) in ("r2", "var")


@add_accessors
@register("org.apache.spark.ml.evaluation.ClusteringEvaluator")
class ClusteringEvaluator(Evaluator, HasFeaturesCol, HasPredictionCol, HasWeightCol, MLWritable, MLReadable):
    """Silhouette with squared euclidean distance (Spark's O(n k) formulation via cluster sums)."""

    metricName = shared("metricName", "metric name in evaluation (silhouette)", TypeConverters.toString)
    distanceMeasure = shared("distanceMeasure", "The distance measure. Supported options: 'squaredEuclidean' "
                                                "and 'cosine'.", TypeConverters.toString)

    @keyword_only
    def __init__(self, *, predictionCol="prediction", featuresCol="features", metricName="silhouette",
                 distanceMeasure="squaredEuclidean", weightCol=None):
        super().__init__()
        self._setDefault(metricName="silhouette", distanceMeasure="squaredEuclidean")
        self._set(**self._input_kwargs)

    def _evaluate(self, df):
        from ..ops import silhouette as SIL
        from .common import dense_features, features_column
        g = self.getOrDefault
        comm = df.comm
        cosine = g(self.distanceMeasure) == "cosine"
        c = _num(df, g(self.predictionCol), None).long()
        k = int(comm.max_scalar(float(c.max().item()) if c.numel() else 0.0)) + 1
        # the fused pass (ops/silhouette.py) reads the stored rows; both paths all-reduce the same
        # two buffers, so ranks may differ in the path they take
        rows = None
        if not cosine and SIL.enabled():
            col = features_column(df, g(self.featuresCol))
            rows = SIL.column_rows(col, k)
            if rows is not None and c.numel() and int(c.min()) < 0:
                rows = None
        if rows is not None:
            D = col.size
            c = c.to(rows.device)
            w = _weights(df, self, rows.shape[0], rows.device, required=False)
            Y, N, Psi = SIL.cluster_moments(rows, c, k, w, D)
            buf = torch.cat([Y.reshape(-1), Psi, N])
        else:
            X = dense_features(df, g(self.featuresCol), torch.float64)
            c = c.to(X.device)
            w = _weights(df, self, X.shape[0], X.device)
            if cosine:
                X = X / X.norm(dim=1, keepdim=True).clamp_min(1e-300)
            D = X.shape[1]
            from ..ops.binsum import bin_sums
            st = bin_sums(X, c, k, w)          # [sum w x | sum w | sum w ||x||^2] per cluster, no atomics
            buf = torch.cat([st[:, :D].reshape(-1), st[:, D + 1], st[:, D]])
        comm.all_reduce(buf)
        Y, Psi, N = buf[: k * D].reshape(k, D), buf[k * D: k * D + k], buf[k * D + k:]
        if rows is not None and int((N > 0).sum()) >= 2:
            s = SIL.silhouette_rows(rows, D, c, Y, N, Psi).double()
            t = torch.stack([s.sum(), s.new_tensor(float(s.numel()))] if w is None else [(s * w).sum(), w.sum()])
        else:
            if rows is not None:               # a single non-empty cluster: the formula's own NaN
                X = rows[:, :D].double()
                w = torch.ones(X.shape[0], dtype=torch.float64, device=X.device) if w is None else w
            s = SIL.silhouette_torch(X, c, k, w, Y, N, Psi, cosine=cosine)
            t = torch.stack([(s * w).sum(), w.sum()])
        comm.all_reduce(t)
        return float(t[0] / t[1])


_ = HasFeaturesCol

from ._evaluation_extra import MultilabelClassificationEvaluator, RankingEvaluator  # noqa: E402,F401
