"""HostFrameStream / PackedFrameStream (app/pipeline.py) as objects of their own.  A per-frame call is a group of one frame
through the code every group takes, so "stream with group 1 == per-frame call" compares that code with itself; here the
one-frame case is pinned to the CPU oracle, and groups, both entry points on one object and the wrap-around of the slot ring
are pinned to it in turn.  Engine and scenes as tests/test_gpu_engine.py builds them: random-init networks carrying
`wire_color_keyed_labels`, colour-keyed synthetic scenes of a few thousand points."""
import numpy as np
import pytest
import torch

from test_gpu_engine_ingest import BOX, _pack_scene

pytestmark = pytest.mark.gpu

SCALE = 50


@pytest.fixture(scope="module")
def engine(gpu):
    import mrcc_amd
    from mrcc_amd.app.inference_engine import InferenceEngine
    from mrcc_amd.utils.config import Config

    Config.reset()
    Config().update({"INFERENCE": {"SEGMENTATION": {"scale": SCALE}}})
    eng = InferenceEngine(allow_random_init=True, seed=3)
    mrcc_amd.synth.wire_color_keyed_labels(eng._segmentation_model)
    yield eng
    Config.reset()


def _stream(engine, cls=None, **kw):
    from mrcc_amd.app.pipeline import HostFrameStream

    kw.setdefault("compute_streams", 1)
    return (cls or HostFrameStream)(engine.device, SCALE, engine._segment, engine._largest_ee_cluster_rule, **kw)


def _scene(seed, n_bg):
    import mrcc_amd
    from mrcc_amd.utils import preprocess

    sc = mrcc_amd.synth.gen_scene(seed, n_bg=n_bg, n_arm=400, n_ee=700, keyed_colors=True)
    return sc["points"], preprocess.normalize_colors(sc["rgb"])


@pytest.fixture(scope="module")
def three(engine, oracle):
    """three frames of different sizes and, computed once, what the oracle's graph followed by the engine's
    largest-cluster rule gives for them: [(points, rgb)], [labels]"""
    frames = [_scene(s, n_bg) for s, n_bg in ((0, 2000), (1, 3100), (2, 2600))]
    sd = {k: v.cpu() for k, v in engine._segmentation_model.state_dict().items()}
    want = []
    for pts, rgb in frames:
        ref = oracle.predict_segmentation(sd, pts, rgb, SCALE)["label"].copy()
        ee = np.where(ref == 2)[0]
        assert len(ee) > 500  # the colour-keyed end effector
        ref[ee] = 1
        ref[ee[engine.cluster_util.get_largest_cluster(pts[ee])]] = 2
        want.append(ref)
    return frames, want


def _same_labels(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == np.int64 and np.array_equal(g, w)


def _check_three(stream, three):
    frames, want = three
    _same_labels([stream.run_one(*f) for f in frames], want)


def test_one_frame_and_groups_equal_the_oracle(engine, three):
    frames, want = three
    _check_three(_stream(engine, one_frame=True), three)  # as predict_segmentation builds its stream
    _check_three(_stream(engine), three)
    for group in (1, 2):
        st = _stream(engine, group=group)
        _same_labels(list(st.run(iter(frames))), want)
        assert st.host_s["frames"] == 3


def test_ring_wraps_with_groups_and_growing_frames(engine):
    """19 frames in groups of 2 over 8 slots: the ring wraps twice and the last group is partial.  The frames grow, and by
    more than the quarter a slot over-reserves (_HostSlot.reserve), so a slot is too small at every reuse and is pinned
    anew behind the wait for its last upload.  float64 points and torch colours are mixed in; every frame's labels are
    those of run_one on a stream object of its own, given the plain float32 / numpy form of the frame."""
    plain = [_scene(10 + i, 1500 + 150 * i) for i in range(19)]
    sizes = [len(p) for p, _ in plain]
    assert all(b > max(a, int(a * 1.25)) for a, b in zip(sizes, sizes[8:]))
    frames = [(p.astype(np.float64) if i % 2 else p, torch.from_numpy(c) if i % 3 == 0 else c)
              for i, (p, c) in enumerate(plain)]
    assert plain[0][0].dtype == np.float32 and not torch.is_tensor(plain[0][1])
    st = _stream(engine, group=2)
    assert len(st._slots) == 8
    got = list(st.run(iter(frames)))
    assert st.host_s["frames"] == 19
    _same_labels(got, [_stream(engine).run_one(*f) for f in plain])
    assert all((g == 2).sum() > 500 for g in got)


def test_both_entry_points_on_one_object(engine, three):
    """run_one, run over five frames in groups of 2, run_one again: one slot counter, one set of streams"""
    frames, want = three
    st = _stream(engine, group=2)
    _same_labels([st.run_one(*frames[1])], want[1:2])
    five = [0, 1, 2, 1, 0]
    _same_labels(list(st.run(iter([frames[i] for i in five]))), [want[i] for i in five])
    _same_labels([st.run_one(*frames[2])], want[2:])
    assert st.host_s["frames"] == 7 and st._n == 7


@pytest.mark.parametrize("group", (1, 4))
def test_an_empty_sequence_yields_nothing(engine, three, group):
    st = _stream(engine, group=group)
    assert list(st.run(iter([]))) == []
    assert st.host_s["frames"] == 0
    _check_three(st, three)


@pytest.fixture(scope="module")
def packed():
    """seven packed frames (frame 3 with a box) and the host arrays they decode to: [(PackedFrame, box)], [(points, rgb)]"""
    import mrcc_amd
    from mrcc_amd.utils import preprocess

    items, hosts = [], []
    for s in range(7):
        scene = mrcc_amd.synth.gen_scene(s, n_bg=1800 + 250 * s, n_arm=400, n_ee=700, keyed_colors=True)
        frame, _ = _pack_scene(scene, s, "kinect32")
        box = BOX if s == 3 else None
        points, rgb, _ = frame.decode_host(box=box)
        items.append((frame, box))
        hosts.append((points, preprocess.normalize_colors(rgb)))
    return items, hosts


def _same_packed(got, items, want):
    assert len(got) == len(items) == len(want)
    for (labels, src), (frame, box), w in zip(got, items, want):
        assert labels.dtype == np.int64 and np.array_equal(labels, w)
        assert src.dtype == np.int32 and np.array_equal(src, frame.decode_host(box=box)[2])


def test_packed_groups_ring_and_both_entry_points(engine, packed):
    """seven frames in groups of 3 on one PackedFrameStream of 12 slots, between two run_one calls and forwards, then
    backwards: 16 frames, so four slots are used a second time, by a frame of another size; labels are the host stream's
    for the decoded arrays (pinned to the oracle above), src the survivors of decode_host"""
    from mrcc_amd.app.pipeline import PackedFrameStream

    items, hosts = packed
    want = [_stream(engine).run_one(*h) for h in hosts]
    assert all((w == 2).sum() > 500 for w in want)
    st = _stream(engine, PackedFrameStream, group=3)
    assert len(st._slots) == 12
    _same_packed([st.run_one(*items[3])], items[3:4], want[3:4])
    _same_packed(list(st.run(iter(items))), items, want)
    _same_packed(list(st.run(iter(items[::-1]))), items[::-1], want[::-1])
    _same_packed([st.run_one(items[0][0])], items[:1], want[:1])
    assert st.host_s["frames"] == 16 and st._n == 16
    assert list(st.run(iter([]))) == []


def test_a_packed_frame_without_a_surviving_record(engine, packed):
    from mrcc_amd.app.pipeline import PackedFrameStream

    items, _ = packed
    nowhere = (items[1][0], (50.0, 50.0, 50.0, 51.0, 51.0, 51.0))
    assert len(nowhere[0].decode_host(box=nowhere[1])[2]) == 0
    st = _stream(engine, PackedFrameStream, group=3)
    with pytest.raises(ValueError, match="inside the box"):
        st.run_one(*nowhere)
    with pytest.raises(ValueError, match="inside the box"):
        list(st.run(iter([items[0], nowhere, items[2]])))
