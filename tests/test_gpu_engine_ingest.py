"""The engine on packed frames: every entry point gives, for a frame that is still the bytes of a PointCloud2 message or of
a .pcd file, what it gives for the host arrays those bytes decode to.  Engine and scenes are those of
tests/test_gpu_engine_icp_batched.py, copied: random-init networks carrying `wire_color_keyed_labels` on colour-keyed
synthetic scenes of a few thousand points (frame 1 has no end effector, frame 2 no ee2base_pose).  Each scene's colours are
quantised to bytes - the keyed colours, >= 0.8 against <= 0.45, survive 8 bits - and packed into an organised cloud with
NaN records interleaved."""
import dataclasses

import numpy as np
import pytest

import ingest_helpers as H

pytestmark = pytest.mark.gpu

CONFIG = {"INFERENCE": {"SEGMENTATION": {"scale": 50}, "ROTATION": {"scale": 100},
                        "KEY_POINTS": {"scale": 100, "conf_threshold": 0.0},
                        "ee_point_counts_threshold": 64, "SANITY": {"min_num_of_ee_points": 64}, "icp_enabled": True}}
WIDTH = 64
BOX = (-2.0, -2.0, -0.5, 2.0, 2.0, 2.6)


def _cad_points():
    rng = np.random.default_rng(77)
    return (rng.uniform(-0.5, 0.5, size=(2048, 3)) * np.array([0.10, 0.22, 0.13]) + np.array([0.0, 0.0, 0.06])).astype(
        np.float32)


@pytest.fixture(scope="module")
def engine(gpu):
    import mrcc_amd
    from mrcc_amd.app.inference_engine import InferenceEngine
    from mrcc_amd.utils.config import Config

    Config.reset()
    Config().update(CONFIG)
    eng = InferenceEngine(allow_random_init=True, seed=3, cad_points=_cad_points(), icp_batched=True)
    mrcc_amd.synth.wire_color_keyed_labels(eng._segmentation_model)
    yield eng
    Config.reset()


def _pack_scene(scene, seed, layout):
    """the scene's points and byte colours as an organised cloud: every third record or so is NaN, the rest are the
    scene's points in order; the last row is filled up with NaN records"""
    rng = np.random.default_rng(seed)
    n = len(scene["points"])
    total = -(-int(n * 1.5) // WIDTH) * WIDTH
    slots = np.sort(rng.permutation(total)[:n])
    xyz = np.full((total, 3), np.nan, dtype=np.float32)
    xyz[slots] = scene["points"]
    c8 = np.round(scene["rgb"] * 255).astype(np.uint32)
    colours = rng.integers(0, 1 << 32, size=total, dtype=np.uint64).astype(np.uint32)
    colours[slots] = (rng.integers(0, 256, size=n).astype(np.uint32) << 24) | (c8[:, 0] << 16) | (c8[:, 1] << 8) | c8[:, 2]
    lay = H.LAYOUTS[layout]
    pad = 12 if layout == "kinect32" else 0
    from mrcc_amd.utils.packed import PackedFrame

    msg = H.Message(H.build(lay, xyz, colours, WIDTH, total // WIDTH, pad), lay, WIDTH, total // WIDTH, pad)
    return PackedFrame.from_pointcloud2(msg), slots


@pytest.fixture(scope="module")
def frames():
    """[(PackedCloudDTO, the PointCloudDTO it decodes to)] - one colour convention and layout for all, as one sensor gives"""
    import mrcc_amd
    from mrcc_amd.app.dto import PackedCloudDTO

    out = []
    for s in range(4):
        scene = mrcc_amd.synth.gen_scene(s, n_bg=5000 + 700 * s, n_arm=700, n_ee=(0 if s == 1 else 1200 + 50 * s),
                                         keyed_colors=True)
        packed, slots = _pack_scene(scene, s, "kinect32")
        dto = PackedCloudDTO(packed=packed, box=(BOX if s == 3 else None), color="float64",
                             ee2base_pose=(None if s == 2 else scene["ee2base_pose"]), id=f"frame{s}")
        host = dto.decoded()
        if s != 3:  # without a box the frame is the scene: same points, in order
            assert np.array_equal(host.points, scene["points"]) and np.abs(host.rgb - scene["rgb"]).max() <= 0.5 / 255 + 1e-7
        else:
            assert 1000 < len(host.points) < len(scene["points"])
        assert host.points.dtype == np.float32 and host.rgb.dtype == np.float64 and host.id == dto.id
        out.append((dto, host, slots))
    return out


def _same_result(o, r):
    """every ResultDTO field"""
    assert [f.name for f in dataclasses.fields(o)] == [f.name for f in dataclasses.fields(r)]
    for f in dataclasses.fields(o):
        a, b = getattr(o, f.name), getattr(r, f.name)
        assert (a is None) == (b is None), f.name
        if a is None:
            continue
        if f.name == "key_points":
            assert len(a) == len(b)
            for (ca, pa), (cb, pb) in zip(a, b):
                assert ca == cb and np.array_equal(pa, pb) and pa.dtype == pb.dtype
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b) and a.dtype == b.dtype, f.name
        else:
            assert a == b, f.name


@pytest.fixture(scope="module")
def reference(engine, frames):
    """per-frame results of the host path, computed once: (labels, ResultDTO)"""
    from mrcc_amd.utils import preprocess

    out = []
    for _, host, _ in frames:
        out.append((engine.predict_segmentation(host.points, preprocess.normalize_colors(host.rgb)), engine.predict(host)))
    assert out[1][1].ee_pose is None and sum(r.ee_pose is not None for _, r in out) == 3
    assert out[2][1].base_pose is None and out[0][1].base_pose is not None
    assert all((labels == 2).sum() > 500 for i, (labels, _) in enumerate(out) if i != 1)
    return out


def test_predict_segmentation_packed(engine, frames, reference):
    for (dto, host, slots), (labels, _) in zip(frames, reference):
        got, src = engine.predict_segmentation_packed(dto.packed, box=dto.box, color=dto.color)
        assert got.dtype == np.int64 and src.dtype == np.int32 and np.array_equal(got, labels)
        assert np.array_equal(src, dto.packed.decode_host(box=dto.box)[2])
        if dto.box is None:
            assert np.array_equal(src, slots)
        image = dto.packed.scatter(got, src)
        assert image.shape == (dto.packed.height, WIDTH) and np.array_equal(image.reshape(-1)[src], labels)
        assert (image == -1).sum() == dto.packed.n_records - len(src)


def test_predict_on_packed_dtos(engine, frames, reference):
    for (dto, _, _), (_, want) in zip(frames, reference):
        _same_result(engine.predict(dto), want)


@pytest.mark.parametrize("pose_thread", (True, False))
def test_predict_stream_on_packed_dtos(engine, frames, reference, pose_thread):
    dtos = [d for d, _, _ in frames]
    for group, seg_group in ((3, 1), (4, 3)):  # neither divides the four frames... nor is divided by them
        out = list(engine.predict_stream(iter(dtos), group=group, seg_group=seg_group, pose_thread=pose_thread))
        assert len(out) == len(reference)
        for o, (_, want) in zip(out, reference):
            _same_result(o, want)


def test_predict_segmentation_stream_on_packed_frames(engine, frames, reference):
    five = frames + frames[:1]  # group = 2 leaves one frame over
    for group in (1, 2):
        items = [(d.packed, d.box) for d, _, _ in five]
        out = list(engine.predict_segmentation_stream(iter(items), group=group))
        assert len(out) == 5
        for (labels, src), (dto, _, _), (want, _) in zip(out, five, (reference + reference[:1])):
            assert np.array_equal(labels, want) and np.array_equal(src, dto.packed.decode_host(box=dto.box)[2])
    # bare PackedFrames, no box
    out = list(engine.predict_segmentation_stream(iter([d.packed for d, _, _ in frames[:3]]), group=2))
    for (labels, _), (want, _) in zip(out, reference[:3]):
        assert np.array_equal(labels, want)
    # host arrays still take the host stream
    from mrcc_amd.utils import preprocess

    hosts = [(h.points, preprocess.normalize_colors(h.rgb)) for _, h, _ in frames[:2]]
    for labels, (want, _) in zip(engine.predict_segmentation_stream(iter(hosts)), reference):
        assert isinstance(labels, np.ndarray) and np.array_equal(labels, want)
    assert list(engine.predict_segmentation_stream(iter(()))) == []


def test_pcd_data_engine_packed_and_host_give_the_same_results(engine, tmp_path):
    """three binary .pcd files with their pose files: PCDDataEngine(packed=True) through predict equals packed=False"""
    import mrcc_amd
    from mrcc_amd.app.data_engine import PCDDataEngine

    lay = H.LAYOUTS["pcd16"]
    for k, s in ((3, 0), (11, 2), (20, 3)):
        scene = mrcc_amd.synth.gen_scene(s, n_bg=4000, n_arm=600, n_ee=1300, keyed_colors=True)
        xyz = scene["points"].copy()
        xyz[::17] = np.nan
        xyz[5] = (700.0, 0.0, 0.0)  # outside the +-500 box
        c8 = np.round(scene["rgb"] * 255).astype(np.uint32)
        n = len(xyz)
        head = ("VERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
        body = H.build(lay, xyz, (c8[:, 0] << 16) | (c8[:, 1] << 8) | c8[:, 2], n, 1)
        (tmp_path / f"{k}.pcd").write_bytes(head.encode("ascii") + body.tobytes())
        e = np.asarray(scene["ee2base_pose"], np.float64)
        np.save(tmp_path / f"{k}_robot2ee_pose.npy", np.concatenate([e[:3], e[4:7], e[3:4]]))  # stored xyzw
        np.save(tmp_path / f"{k}.npy", np.zeros(7))
    host_engine = PCDDataEngine(str(tmp_path), cyclic=False, step=1)
    packed_engine = PCDDataEngine(str(tmp_path), cyclic=False, step=1, packed=True)
    assert len(host_engine) == len(packed_engine) == 3
    for _ in range(3):
        host, packed = host_engine.get(), packed_engine.get()
        assert host.id == packed.id and host.rgb.dtype == np.float32
        want = engine.predict(host)
        assert want.ee_pose is not None and want.base_pose is not None and len(want.segmentation) == len(host.points)
        _same_result(engine.predict(packed), want)
    assert host_engine.get() is None and packed_engine.get() is None
