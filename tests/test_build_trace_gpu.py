"""The scratch choreography of the three device builders (build_ivf_index_device, build_ivfpq_index_device,
build_ivfsq_index_device) is behaviour: whether BASELINE config 5's 256 GB shard fits one card depends on the sample being freed
before the list and row buffers exist, on the rotation buffer going before the arena comes, and so on.  Every builder runs here with
an `alloc` hook that logs ("alloc", nbytes), hands out a keep-alive object whose finaliser logs ("free", nbytes), and a `fill_rows`
that logs ("fill", row0, count, stride); the event list must be the one recorded in tests/golden/build_trace/events.json.

That file was recorded by running trace() of this module on the commit before the builders were put on one driver (a96eae1), never
computed by code that restates the driver: tests/golden/build_trace/README.md."""
import json
import os

import pytest

from build_cases import CHUNK, D, M, N, NLIST, corpus, fill_rows

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_trace", "events.json")

# case -> (kind, what the builder is given beyond the shape)
CASES = {
    "flat-trained": ("flat", {}),
    "flat-trained-keep-lists": ("flat", {"keep_lists": True}),
    "pq-given": ("pq", {"given": True}),
    "pq-trained": ("pq", {}),
    "pq-given-rotation": ("pq", {"given": True, "rotation": "rotation"}),
    "pq-trained-rotation": ("pq", {"rotation": "rotation"}),
    "pq-trained-rect-rotation": ("pq", {"rotation": "rect"}),  # (the rotated chunk is twice as wide as the generated one)
    "pq-given-refine": ("pq", {"given": True, "refine": True}),
    "sq-given": ("sq", {"given": True}),
    "sq-trained": ("sq", {}),
}


class _Keep:
    """What the alloc hook returns next to the pointer: owns the buffer, logs when the builder lets go of it."""

    def __init__(self, events, tensor, nbytes):
        self.events, self.tensor, self.nbytes = events, tensor, nbytes

    def __del__(self):
        self.events.append(["free", self.nbytes])


def trace(case):
    """The event list of one build: [["alloc", nbytes] | ["free", nbytes] | ["fill", row0, count, stride], ...]."""
    import torch

    from clip_retrieval_amd import knn

    kind, opt = CASES[case]
    c = corpus()
    events = []

    def alloc(nbytes):
        events.append(["alloc", int(nbytes)])
        t = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda:0")
        return t.data_ptr(), _Keep(events, t, int(nbytes))

    def fill(dst, row0, count, stride):
        events.append(["fill", int(row0), int(count), int(stride)])
        fill_rows(dst, row0, count, stride)

    kw = dict(nprobe=NLIST, chunk=CHUNK, alloc=alloc, seed=3)
    if kind == "flat":
        index, stats = knn.build_ivf_index_device(fill, N, D, NLIST, keep_lists=opt.get("keep_lists", False), **kw)
        assert sorted(stats) == sorted(["train_s", "assign_s", "scatter_s", "n_sample", "list_sizes"])
    elif kind == "pq":
        if opt.get("given"):
            kw.update(centroids=c["cent"], codebooks=c["codebooks"])
        index, stats = knn.build_ivfpq_index_device(fill, N, D, NLIST, M, rotation=c[opt["rotation"]] if "rotation" in opt else None,
                                                    refine=opt.get("refine", False), **kw)
        assert sorted(stats) == sorted(["train_s", "assign_s", "encode_s", "list_sizes", "bytes_per_row", "rotate_s", "opq_s",
                                        "code_arena_bytes", "row_arena_bytes"])
    else:
        if opt.get("given"):
            kw.update(centroids=c["cent"], ranges=c["ranges"])
        index, stats = knn.build_ivfsq_index_device(fill, N, D, NLIST, **kw)
        assert sorted(stats) == sorted(["train_s", "assign_s", "encode_s", "list_sizes", "bytes_per_row", "arena_bytes"])
    assert index.ntotal == N and int(stats["list_sizes"].sum()) == N
    assert hasattr(index, "ivf_centroids") == (kind != "flat")  # the flat device builder never recorded them
    assert hasattr(index, "ivf_lists") == bool(opt.get("keep_lists"))
    index.close()
    return events


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_builder_events_are_the_recorded_ones(case):
    with open(GOLDEN, encoding="utf-8") as f:
        expected = json.load(f)[case]
    got = trace(case)
    print(f"{case}: {len(got)} events")
    assert ["fill", 4000, 1000, 1] in got  # the ragged last chunk
    assert sum(e[0] == "alloc" for e in got) == sum(e[0] == "free" for e in got), "a scratch buffer outlived the build"
    for i, (a, b) in enumerate(zip(got, expected)):
        assert a == b, f"{case}: event {i} is {a}, recorded {b}"
    assert len(got) == len(expected), f"{case}: {len(got)} events, recorded {len(expected)}"
