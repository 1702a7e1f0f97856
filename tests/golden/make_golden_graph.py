#!/usr/bin/env python3
"""F11: graph-neighbour golden vectors from the REFERENCE's own ``build_index`` / ``expand_qmatch_neighbors``
(app/modules/retrieval/graph_utils.py:25-129) on seeded chain graphs: documents whose sentences are linked by
``next_in_doc`` edges in sentence order (edge_builder.py:106-120), the question's ``q_match`` edges as the seeds.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_golden_graph.py

The script only CALLS the reference; the fixture holds inputs and its outputs.  Per case: the document lengths (row r of
the corpus is the r-th sentence when the documents stand one after the other), the seed rows (duplicates kept as drawn),
the window, and ``{row: [score, distance]}`` as the reference returned it.
"""
import json
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from app.modules.retrieval.graph_utils import build_index, expand_qmatch_neighbors  # noqa: E402  (reference)


def chain_graph(doc_lens, seed_rows):
    """the graph.json shape GraphConstructionNetworkX writes: sentence nodes, next_in_doc edges, q_match edges from q1"""
    nodes, edges, node_of = [{"id": "q1", "type": "question", "props": {"text": "q"}}], [], []
    for d, n in enumerate(doc_lens):
        for i in range(n):
            nid = f"Doc {d}::{i}"
            nodes.append({"id": nid, "type": "sentence", "props": {"text": f"sentence {i} of {d}", "doc": f"Doc {d}"}})
            if i:
                edges.append({"type": "next_in_doc", "source": node_of[-1], "target": nid})
            node_of.append(nid)
    for r in seed_rows:
        edges.append({"type": "q_match", "source": "q1", "target": node_of[r]})
    return {"nodes": nodes, "edges": edges}, node_of


def capture(doc_lens, seed_rows, window):
    graph, node_of = chain_graph(doc_lens, seed_rows)
    nodes_by_id, nf, nb, texts, qmatch = build_index(graph)
    got = expand_qmatch_neighbors("q", nodes_by_id, nf, nb, texts, explicit_qmatch=qmatch, window=window)
    row_of = {nid: r for r, nid in enumerate(node_of)}
    return {"doc_lens": doc_lens, "seeds": seed_rows, "window": window,
            "expanded": {str(row_of[sid]): [float(sc), int(meta["distance"])] for sid, (sc, meta) in sorted(got.items(), key=lambda kv: row_of[kv[0]])}}


def main():
    rng = random.Random(11)
    cases = []
    for window in range(9):
        for n_docs in range(1, 7):
            for _ in range(2):
                doc_lens = [rng.randint(1, 7) for _ in range(n_docs)]
                n = sum(doc_lens)
                first = [sum(doc_lens[:d]) for d in range(n_docs)]
                seeds = [rng.randrange(n) for _ in range(rng.randint(1, 5))]
                d = rng.randrange(n_docs)
                seeds += [first[d], first[d] + doc_lens[d] - 1]           # both ends of one document
                seeds.append(seeds[rng.randrange(len(seeds))])            # a duplicate seed
                rng.shuffle(seeds)
                cases.append(capture(doc_lens, seeds, window))
    # worked by hand: all documents of lengths 1 .. 7 in a row, one seed at the first row, one at the last, one in the middle
    lens = [1, 2, 3, 4, 5, 6, 7]
    for window in (0, 1, 2, 3, 5, 8):
        cases.append(capture(lens, [0, 27, 12, 12], window))
    dst = HERE / "f11_graph_neighbors.json"
    dst.write_text(json.dumps({"cases": cases}, separators=(",", ":")))
    print("wrote", dst, dst.stat().st_size, "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
