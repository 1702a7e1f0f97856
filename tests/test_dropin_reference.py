"""Drop-in check against what the REAL reference classes do with this package (fixture F10,
tests/golden/make_golden_dropin.py): the reference's own factory / router / re-ranker / adapter were driven with this
repo's provider and backend selected by "pkg.mod:Class" strings, exactly as config/settings.yaml would, and every call
they made on our objects was recorded with what our objects returned.  Here those calls are replayed on our classes:
the same calls must give the same returns."""
import importlib
import json
import sys
import types
from types import SimpleNamespace

import numpy as np
import pytest


def _import_from_string(spec):
    mod, _, name = spec.partition(":")
    return getattr(importlib.import_module(mod), name)


def _fixture(golden_dir):
    return json.loads((golden_dir / "f10_dropin.json").read_text())


def test_reference_factory_builds_our_provider_and_router_calls_it(golden_dir, monkeypatch):
    fx = _fixture(golden_dir)["provider"]
    from mrag_amd.provider import HipEmbeddingProvider
    Cls = _import_from_string(fx["settings"]["providers"]["hip"]["type"])
    assert Cls is HipEmbeddingProvider
    # the reference factory (factory.py:32-58) built the provider through from_settings(settings) -- it did not raise --
    # which constructed it with the provider entry's kwargs
    (fs,) = fx["calls"]["from_settings"]
    assert fs["outcome"] == "ok" and fs["settings"] == fx["settings"]
    inits, orig_init = [], Cls.__init__

    def init(self, *a, **kw):
        inits.append({"args": list(a), "kwargs": kw})
        orig_init(self, *a, **kw)
    monkeypatch.setattr(Cls, "__init__", init)
    provider = Cls.from_settings(fs["settings"])
    assert isinstance(provider, HipEmbeddingProvider) and inits == fx["calls"]["init"]
    assert provider.kwargs["embed_model"] == "tiny-seed0"
    # the reference's DenseReranker resolved the embedding model from provider.kwargs
    assert fx["reranker_resolved_model"] == provider.kwargs["embed_model"]
    seen = []

    def fake_embed_array(self, texts):                               # no GPU here: stub only the forward pass
        seen.append(list(texts))
        return np.ones((len(texts), 4), dtype=np.float32)
    monkeypatch.setattr(HipEmbeddingProvider, "embed_array", fake_embed_array)
    # every embed call of the reference router (llm_router.py:115), for itself and for the re-ranker, in order
    for call in fx["calls"]["embed"]:
        assert provider.embed(*call["args"], **call["kwargs"]) == call["returned"]
    assert seen == [["a", "b"], ["q"], ["hello"]] == [c["kwargs"]["texts"] for c in fx["calls"]["embed"]]
    # ... and what the reference made of those returns: the router passed ours through, the re-ranker scored with it
    out = fx["router_embed_out"]
    assert out == fx["calls"]["embed"][0]["returned"] and len(out["vectors"]) == 2 and out["vectors"][0] == [1.0] * 4
    assert fx["reranker_scores"] == {"x": pytest.approx(1.0)}


def test_reference_adapter_drives_our_backend(golden_dir, tmp_path, monkeypatch):
    fx = _fixture(golden_dir)["backend"]
    from mrag_amd.backend import DenseRetrievalBackend
    from mrag_amd.dto import RetrievalIn
    # the reference's RetrievalAdapter built the backend as BackendCls(router=..., sink=..., **backend_kwargs) around an
    # LLMRouter(providers={}, policy={}); the backend reads only those two attributes of it
    (init,) = fx["calls"]["init"]
    assert init["args"] == 0 and init["kwargs"]["router"] == "<router>"
    router = SimpleNamespace(**fx["router"])
    kw = dict(init["kwargs"], router=router, index_path=str(tmp_path / init["kwargs"]["index_path"]))
    backend = _import_from_string("mrag_amd.backend:DenseRetrievalBackend")(**kw)
    assert isinstance(backend, DenseRetrievalBackend)
    (run,) = fx["calls"]["run"]
    assert run["req_type"] == "app.core.dto.RetrievalIn"
    got = backend.run(RetrievalIn(**run["req"]))
    want = run["returned"]
    assert got["hits"] == want["hits"] == []
    assert {k: got["diagnostics"].get(k) for k in want["diagnostics"]} == want["diagnostics"]
    assert fx["adapter_out"] == {"hits": [], "resolved_embed_model": "text-embedding-3-large", "dense_error": None}
    assert got["diagnostics"]["resolved_embed_model"] == fx["adapter_out"]["resolved_embed_model"]
    # our agent returns the REFERENCE's DTO classes when they are importable (app.core.dto on sys.path)
    import mrag_amd.dto as d
    with monkeypatch.context() as m:
        for name in ("app", "app.core", "app.core.dto"):
            m.setitem(sys.modules, name, types.ModuleType(name))
        ref_dto = sys.modules["app.core.dto"]
        for name in ("Hit", "RetrievalIn", "RetrievalOut"):
            setattr(ref_dto, name, type(name, (), {}))
        importlib.reload(d)
        assert d.USING_REFERENCE_DTO and d.RetrievalOut is ref_dto.RetrievalOut and d.RetrievalIn is ref_dto.RetrievalIn
    importlib.reload(d)
    assert not d.USING_REFERENCE_DTO
