"""Headless widget integration: replay the tutorial graph (reference
orangecontrib/spark/tutorials/spark_ml.ows) and exercise every widget's inputs -> outputs."""
import os

import numpy as np
import pandas as pd
import pytest

from orangecontrib.spark_amd.utils.gui_param import GuiParam, coerce
from orangecontrib.spark_amd.utils import ml_api_utils as R
from orangecontrib.spark_amd.widgets.base import SharedSession
from orangecontrib.spark_amd.workflow import Workflow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUTORIAL = os.path.join(ROOT, "orangecontrib", "spark_amd", "tutorials", "spark_ml.ows")


@pytest.fixture()
def warehouse(tmp_path):
    SharedSession._session = None
    yield str(tmp_path / "wh")
    from orange3_spark_amd import Session
    if SharedSession._session is not None:
        SharedSession._session.stop()
    SharedSession._session = None
    Session._active = None


def test_gui_param_coercion_rules():
    # reference gui_utils.py:78-94
    assert coerce("None") is None and coerce("") is None
    assert coerce("True") is True and coerce("False") is False
    assert coerce("5") == 5 and isinstance(coerce("5"), int)
    assert coerce("1.0") == 1.0 and isinstance(coerce("1.0"), float)
    assert coerce("1e-6") == 1e-6
    assert coerce("abc") == "abc"
    assert coerce("[a, b]") == ["a", "b"] and coerce("[0.5, 1]") == [0.5, 1]   # Q11 extension
    p = GuiParam(label="x", default_value="True")
    assert p.gui_type == "multiple" and p.list_values == ["True", "False"]
    p.set_value("False")
    assert p.get_usable_value() is False


def test_reflection_contract():
    from orange3_spark_amd.ml import classification, evaluation, feature
    est = R.get_estimators(None, classification)
    assert {"LogisticRegression", "LinearSVC", "GBTClassifier", "RandomForestClassifier"} <= set(est)
    tr = R.get_transformers(None, feature)
    assert "VectorAssembler" in tr and "HashingTF" in tr and "StandardScaler" not in tr
    ev = R.get_evaluators(None, evaluation)
    assert "BinaryClassificationEvaluator" in ev and "Evaluator" not in ev
    name, doc, params, html = R.get_object_info(est["LogisticRegression"])
    assert list(params)[:3] == ["featuresCol", "labelCol", "predictionCol"]
    assert params["maxIter"][1] == 100 and "iterations" in params["maxIter"][2]
    bce = ev["BinaryClassificationEvaluator"]()
    doc = bce.getParam("metricName").doc
    assert doc.split("(")[-1].replace(")", "").split("|") == ["areaUnderROC", "areaUnderPR"]


def _make_tables(session):
    rng = np.random.default_rng(0)
    for name, n in (("train", 1500), ("test", 500)):
        X = rng.normal(size=(n, 6))
        y = (X @ [1.0, -1.0, 0.5, 0.0, 2.0, -0.5] + rng.normal(scale=0.5, size=n) > 0).astype(int)
        pdf = pd.DataFrame(X, columns=[f"f{i}" for i in range(6)])
        pdf["outcome"] = y
        pdf["comment"] = ["c%d" % (i % 3) for i in range(n)]
        session.createDataFrame(pdf).write.mode("overwrite").saveAsTable(name)


def test_tutorial_workflow_end_to_end(warehouse):
    wf = Workflow.load(TUTORIAL).instantiate()
    ctx = wf.widget("Context")
    ctx.set_param("o3s.device", "cpu").set_param("spark.sql.warehouse.dir", warehouse)
    s = ctx.create_context()
    _make_tables(s)
    for title in ("Training data", "Testing Data"):
        w = wf.widget(title)
        w.refresh()
        assert "default" in w.databases and {"train", "test"} <= set(w.tables)
        w.submit()
    for title in ("Dataset Builder", "Dataset Builder (1)"):
        b = wf.widget(title)
        b.set_features([f"f{i}" for i in range(6)])
        b.set_label("outcome")
        b.set_metas(["comment"])
        b.commit()
    clf = wf.widget("Classification")
    clf.select_method("LogisticRegression").set_param("maxIter", "50").set_param("regParam", "None")
    model = clf.apply()
    assert model is not None, clf.messages
    mt = wf.widget("Model Transformer")
    assert mt.out_df is not None and "prediction" in mt.out_df.columns and "comment" in mt.out_df.columns
    ev = wf.widget("Evaluation")
    ev.select_method("BinaryClassificationEvaluator")
    vals = ev.apply()
    assert set(vals) == {"areaUnderROC", "areaUnderPR"} and vals["areaUnderROC"] > 0.9
    # settings round-trip through a saved workflow
    out = os.path.join(os.path.dirname(warehouse), "saved.ows")
    wf.save(out)
    wf2 = Workflow.load(out)
    assert wf2.nodes["3"].properties["saved_gui_params"]["maxIter"] == "50"


def test_reference_tutorial_graph_maps_to_our_widgets(warehouse):
    ref = "/root/reference/orangecontrib/spark/tutorials/spark_ml.ows"
    if not os.path.exists(ref):
        pytest.skip("reference checkout not present")
    wf = Workflow.load(ref).instantiate()      # pickle properties are skipped, never unpickled
    assert type(wf.widget("Evaluation")).__name__ == "OWEvaluation"
    assert len(wf.links) == 6


def test_pickle_format_properties_are_skipped_with_a_warning(warehouse, tmp_path, caplog):
    # this add-on's tutorial with every node renamed through the inverse of REFERENCE_WIDGETS
    # (so the names are the table's own, not an independent check of it) and the properties of
    # three nodes stored as an opaque pickle-format blob: each must be skipped, never loaded
    import base64
    import xml.etree.ElementTree as ET
    from orangecontrib.spark_amd.workflow import REFERENCE_WIDGETS
    upstream = {ours: theirs for theirs, ours in REFERENCE_WIDGETS.items()}
    root = ET.parse(TUTORIAL).getroot()
    for n in root.iter("node"):
        qn = n.get("qualified_name")
        n.set("qualified_name", upstream[qn[:-4] if qn.endswith("View") else qn])
        n.set("project_name", "Orange3-spark")
    for p in root.iter("properties"):
        if p.get("node_id") in ("0", "3", "7"):
            p.set("format", "pickle")
            p.text = base64.encodebytes(b"\x80\x03not a pickle anyone may load\x00.").decode()
    ref = str(tmp_path / "upstream_spark_ml.ows")
    ET.ElementTree(root).write(ref, encoding="utf-8", xml_declaration=True)
    assert all(n.get("qualified_name").startswith("orangecontrib.spark.widgets.") for n in root.iter("node"))
    with caplog.at_level("WARNING", logger="orangecontrib.spark_amd.workflow"):
        wf = Workflow.load(ref).instantiate()      # pickle properties are skipped, never unpickled
    assert sum("never unpickled" in r.getMessage() for r in caplog.records) == 3
    assert type(wf.widget("Evaluation")).__name__ == "OWEvaluation"
    assert len(wf.links) == 6


def test_data_widgets(warehouse):
    from orangecontrib.spark_amd.widgets.data import (owcache, owcontext, owdatabase, owfillna, owfromorange,
                                                      owfrompandas, owpandastoorange, owsample, owscript, owsql,
                                                      owtoorange, owtopandas, oworangetopandas)
    ctx = owcontext.OWSessionContext()
    ctx.set_param("o3s.device", "cpu").set_param("spark.sql.warehouse.dir", warehouse)
    s = ctx.create_context()
    pdf = pd.DataFrame({"a": [1.0, np.nan, 3.0], "b": ["x", None, "z"]})
    fp = owfrompandas.OWFromPandas()
    df = fp.get_input(pdf)
    fill = owfillna.OWFillNa(value="0", subset="a")
    fill.get_input(df)
    out = fill.apply()
    assert out.toPandas()["a"].tolist() == [1.0, 0.0, 3.0]
    samp = owsample.OWSample(fraction="1.0")
    samp.get_input(df)
    assert samp.apply().count() == 3
    cache = owcache.OWCacheDataFrame()
    cache.get_input(df)
    assert cache.sent["DataFrame"].is_cached
    t = owtoorange.OWToOrange().get_input(df)
    assert [v.name for v in t.domain.attributes] == ["a"]
    back = owfromorange.OWFromOrange().get_input(t)
    assert back.count() == 3
    assert owtopandas.OWToPandas().get_input(df).shape == (3, 2)
    t2 = owpandastoorange.OWPandasToOrange().get_input(pdf)
    assert oworangetopandas.OWOrangeToPandas().get_input(t2).shape == (3, 2)
    df.createOrReplaceTempView("tmp")
    q = owsql.OWSQLDataFrame()
    assert q.format_query("select a from tmp where a > 1").startswith("SELECT")
    assert q.execute("select a from tmp where a >= 1").count() == 2
    sc = owscript.OWScript(scriptText="out_object = in_object.count() * 10")
    sc.set_in_object(df)
    sc.handleNewSignals()
    assert sc.sent["out_object"] == 30            # Q4: read back from the namespace
    db = owdatabase.OWDatabase()
    db.connect()
    db.conn.execute("create table t (x real, y text)")
    db.conn.executemany("insert into t values (?, ?)", [(1.5, "a"), (2.5, "b")])
    got = db.execute_query("select * from t")
    assert got.shape == (2, 2) and db.sent["Data"].X.shape == (2, 1)


def test_ml_widgets_pipeline_tuning_modelio(warehouse, tmp_path):
    from orangecontrib.spark_amd.widgets.compat import SignalManager
    from orangecontrib.spark_amd.widgets.data import owcontext
    from orangecontrib.spark_amd.widgets.ml import (owclustering, owfeature, owfeatureestimator, owmodelio,
                                                    owpipeline, owtuning, owclassification)
    ctx = owcontext.OWSessionContext()
    ctx.set_param("o3s.device", "cpu").set_param("spark.sql.warehouse.dir", warehouse)
    s = ctx.create_context()
    rng = np.random.default_rng(1)
    X = rng.normal(size=(600, 4))
    pdf = pd.DataFrame(X, columns=list("abcd"))
    pdf["label"] = (X[:, 0] + X[:, 1] > 0).astype(float)
    df = s.createDataFrame(pdf)
    sm = SignalManager()
    va = sm.add(owfeature.OWFeature())
    va.select_method("VectorAssembler").set_param("inputCols", "[a, b, c, d]").set_param("outputCol", "raw")
    sc = sm.add(owfeatureestimator.OWFeatureEstimator())
    sc.select_method("StandardScaler").set_param("inputCol", "raw").set_param("outputCol", "features")
    lr = sm.add(owclassification.OWClassification())
    lr.select_method("LogisticRegression")
    pipe = sm.add(owpipeline.OWPipeline())
    for w in (va, sc, lr):
        sm.link(w, "Stage", pipe, "Stage")
    va.apply(), sc.apply(), lr.apply()                  # no DataFrame yet: emit configured stages
    assert [type(x).__name__ for x in pipe.stages.values()] == ["VectorAssembler", "StandardScaler", "LogisticRegression"]
    pipe.stages.clear()
    for i, w in enumerate((va, sc, lr)):
        pipe.add_stage(w.sent["Stage"], key=i)
    pipe.set_data(df)
    pm = pipe.apply()
    assert pm is not None, pipe.messages
    pred = pm.transform(df).toPandas()["prediction"].values
    assert (pred == pdf["label"].values).mean() > 0.95
    io = owmodelio.OWModelIO(path=str(tmp_path / "pm"))
    io.set_model(pm)
    io.save()
    loaded = io.load()
    assert type(loaded).__name__ == "PipelineModel"
    km = owclustering.OWClustering()
    km.get_input(pm.stages[0].transform(df))
    km.select_method("KMeans").set_param("k", "3").set_param("featuresCol", "raw")
    assert km.apply().summary.k == 3
    from orange3_spark_amd.ml.evaluation import BinaryClassificationEvaluator
    tune = owtuning.OWTuning(grid={"regParam": "[0.0, 0.1]"})
    feat = pm.stages[1].transform(pm.stages[0].transform(df))
    tune.set_stage(lr.sent["Stage"])
    tune.set_evaluator(BinaryClassificationEvaluator())
    tune.set_data(feat)
    m = tune.apply()
    assert len(tune.metrics) == 2 and m.bestModel is not None


def test_csv_io_roundtrip_fixes_reference_quirks():
    """save_csv_IO / load_csvIO: the reference's versions raised (empty delimiter) and returned
    nothing (lazy map) -- quirks Q1/Q2; here they round-trip an Orange table."""
    import pandas as pd
    from orange3_spark_amd.utils.data_utils import load_csvIO, pandas_to_orange, save_csv_IO
    t = pandas_to_orange(pd.DataFrame({"a": [1.5, 2.0, 3.25], "k": [1, 2, 1], "s": ["x", None, "z"]}))
    header, rows = load_csvIO(save_csv_IO(t))
    assert header == ["a", "k", "s"]
    assert rows[0][0] == 1.5 and rows[1][2] is None and rows[2][2] == "z"


def test_tutorial_has_reference_layout_and_annotations():
    """The shipped tutorial places its 8 nodes where the reference does
    (orangecontrib/spark/tutorials/spark_ml.ows:4-11) and carries its instructional
    annotations (:22-37), so the canvas opens a readable workflow."""
    import ast
    import os
    import xml.etree.ElementTree as ET
    from orangecontrib.spark_amd.workflow import Workflow
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "orangecontrib", "spark_amd", "tutorials", "spark_ml.ows")
    tree = ET.parse(path).getroot()
    pos = [ast.literal_eval(n.get("position")) for n in tree.iter("node")]
    assert len(pos) == 8 and len(set(pos)) == 8
    assert dict(zip([n.get("title") for n in tree.iter("node")], pos))["Evaluation"] == (641.0, 397.0)
    texts = " ".join(t.text for t in tree.iter("text"))
    for phrase in ("First, create the session", "features and the label column", "obtain a fitted model",
                   "Apply the fitted model to the testing dataset", "measures"):
        assert phrase in texts
    assert len(list(tree.iter("arrow"))) == 7
    wf = Workflow.load(path)                       # positions / annotations round-trip
    assert wf.nodes["3"].position == (341.0, 247.0) and len(wf.annotations) == 13


def test_context_widget_keeps_environment_keys(monkeypatch, warehouse):
    """Context widget (reference spark_context.py:31-32,52-58): keys the configuration
    already holds (O3S_CONF_* environment) appear in the editor and reach the session;
    camelCase keys keep their case."""
    from orange3_spark_amd.conf import SessionConf, env_key
    from orangecontrib.spark_amd.widgets.data import owcontext
    from orange3_spark_amd import Session
    from orangecontrib.spark_amd.widgets.base import SharedSession
    monkeypatch.setattr(Session, "_active", None)
    monkeypatch.setattr(SharedSession, "_session", None)
    monkeypatch.setenv("O3S_CONF_o3s__executor__commTimeout", "7")
    monkeypatch.setenv("O3S_CONF_O3S__SEED", "123")
    assert env_key("O3S_CONF_o3s__executor__commTimeout") == "o3s.executor.commTimeout"
    assert env_key("O3S_CONF_SPARK__EXECUTOR__INSTANCES") == "spark.executor.instances"
    assert SessionConf().get("o3s.executor.commTimeout") == "7"
    ctx = owcontext.OWSessionContext()
    assert ctx.gui_parameters["o3s.executor.commTimeout"].get_value() == "7"
    assert ctx.gui_parameters["o3s.seed"].get_value() == "123"
    ctx.set_param("o3s.device", "cpu").set_param("spark.sql.warehouse.dir", warehouse)
    s = ctx.create_context()
    try:
        assert s.conf.get("o3s.executor.commTimeout") == "7"
        assert s.conf.get("o3s.seed") == "123"
        assert ctx.saved_gui_params["o3s.executor.commTimeout"] == "7"
    finally:
        ctx.onDeleteWidget()
