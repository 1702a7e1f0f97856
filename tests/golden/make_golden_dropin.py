#!/usr/bin/env python3
"""F10: what the REFERENCE's own plug-in machinery does with this package's classes when its settings select them
by "pkg.mod:Class" strings (app/di/factory.py build_providers / build_router, app/core/llm_router.py LLMRouter.embed,
retrieval_backend.py DenseReranker, retrieval_adapter.py RetrievalAdapter).  Every call the reference makes on our
provider / backend is recorded with its arguments and what our object returned, plus the reference-side results.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_golden_dropin.py

The script only CALLS the reference; the fixture holds the calls and values (tests/test_dropin_reference.py replays them).
"""
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from app.core.dto import RetrievalIn                                      # noqa: E402  (reference)
from app.core.llm_router import LLMRouter                                # noqa: E402
from app.di.factory import build_providers, build_router                 # noqa: E402
from app.modules.retrieval.retrieval_adapter import RetrievalAdapter     # noqa: E402
from app.modules.retrieval.retrieval_backend import DenseReranker        # noqa: E402

from mrag_amd.backend import DenseRetrievalBackend                       # noqa: E402
from mrag_amd.provider import HipEmbeddingProvider                       # noqa: E402

TIME_KEYS = ("_ms", "_s", "latency", "duration", "seconds")


def provider_case():
    calls = {"from_settings": [], "init": [], "embed": []}
    orig_fs, orig_init, orig_embed = HipEmbeddingProvider.from_settings.__func__, HipEmbeddingProvider.__init__, HipEmbeddingProvider.embed

    def fs(cls, settings):
        try:
            inst = orig_fs(cls, settings)
        except Exception as e:
            calls["from_settings"].append({"settings": settings, "outcome": "raised", "error": type(e).__name__})
            raise
        calls["from_settings"].append({"settings": settings, "outcome": "ok"})
        return inst

    def init(self, *a, **kw):
        calls["init"].append({"args": list(a), "kwargs": kw})
        orig_init(self, *a, **kw)

    def embed(self, *a, **kw):
        out = orig_embed(self, *a, **kw)
        calls["embed"].append({"args": list(a), "kwargs": kw, "returned": out})
        return out

    HipEmbeddingProvider.from_settings = classmethod(fs)
    HipEmbeddingProvider.__init__ = init
    HipEmbeddingProvider.embed = embed
    HipEmbeddingProvider.embed_array = lambda self, texts: np.ones((len(texts), 4), dtype=np.float32)   # no GPU: forward stubbed
    settings = {"providers": {"hip": {"type": "mrag_amd.provider:HipEmbeddingProvider",
                                      "kwargs": {"arch": "tiny", "embed_model": "tiny-seed0", "seed": 0}}},
                "llm_policy": {"embedding_provider": "hip"}}
    providers = build_providers(settings)
    router = build_router(settings, providers)
    router_out = router.embed(model_hint="tiny-seed0", texts=["a", "b"], require={"trace_id": "t"})
    rr = DenseReranker(router, max_pool=5, embed_batch=8)
    resolved = rr._resolve_embed_model()
    scores = rr.score(query="q", candidates=[{"id": "x", "score": 1.0, "meta": {"text": "hello"}}], trace_id="t")
    return {"settings": settings, "calls": calls, "router_embed_out": router_out, "reranker_resolved_model": resolved,
            "reranker_scores": scores}


def backend_case():
    calls = {"init": [], "run": []}
    orig_init, orig_run = DenseRetrievalBackend.__init__, DenseRetrievalBackend.run

    def init(self, *a, **kw):
        rec = {k: ("<router>" if k == "router" and v is not None else v) for k, v in kw.items()}
        rec["index_path"] = Path(rec["index_path"]).name
        calls["init"].append({"args": len(a), "kwargs": rec})
        orig_init(self, *a, **kw)

    def run(self, req):
        out = orig_run(self, req)
        calls["run"].append({"req": req.model_dump(), "req_type": f"{type(req).__module__}.{type(req).__name__}",
                             "returned": {"hits": out["hits"],
                                          "diagnostics": {k: v for k, v in out["diagnostics"].items()
                                                          if not any(t in k for t in TIME_KEYS)}}})
        return out

    DenseRetrievalBackend.__init__ = init
    DenseRetrievalBackend.run = run
    with tempfile.TemporaryDirectory() as d:
        router = LLMRouter(providers={}, policy={})
        ad = RetrievalAdapter(router=router, backend_impl="mrag_amd.backend:DenseRetrievalBackend",
                              backend_kwargs={"index_path": str(Path(d) / "no-docs.jsonl")})
        out = ad.retrieve(RetrievalIn(query="q", graph_id="", top_k=3, trace_id="t"))
    return {"router": {"providers": {}, "policy": {}}, "calls": calls,
            "adapter_out": {"hits": [h.model_dump() for h in out.hits], "resolved_embed_model": out.diagnostics["resolved_embed_model"],
                            "dense_error": out.diagnostics["dense_error"]}}


if __name__ == "__main__":
    fx = {"note": "F10: the reference's plug-in machinery driving this package's provider and backend (make_golden_dropin.py)",
          "provider": provider_case(), "backend": backend_case()}
    dst = Path(__file__).resolve().parent / "f10_dropin.json"
    dst.write_text(json.dumps(fx, indent=1, sort_keys=True) + "\n")
    print(f"wrote {dst}")
