"""What turning a depth image and a colour image into a cloud costs, on the host and on the device.  The comparison side
is the numpy restatement of the same run (RGBDFrame.decode_host: vectorised, already far quicker than the reference's
per-pixel Python loops).  Each section runs in a child process of its own under `timeout`, one after the other; the first
that fails ends the run.

    python tools/rgbd_timing.py [--frames 32] [--sections decode,host,rgbd,take,lens] [--group 1]

decode:  RGBDFrame.decode_device (staging copy, upload, sv_rgbd_cloud, 8-byte read-back) against decode_host at 480 x 640
         and 720 x 1280, registered and aligned, the 7 x 7 filter on and off; and sv_rgbd_cloud alone on resident bytes
         between two stream events.
host:    decode_host + normalize_colors feeding InferenceEngine.predict_segmentation_stream: frames/s and the host
         milliseconds per frame spent decoding.
rgbd:    the same frames as RGBDFrame items through the packed stream: frames/s and the stream's host stage.
         The scene is a surface seen from one side: about 7 000 voxels at 2 cm against the 88 000 of bench.py's room, a
         small network run, so the frames/s of both sides show the host's share and are not comparable with bench.py's.
take:    what the pose stages' crop costs on a registered frame: the first take() runs the host registration, later ones
         read the cached map.
lens:    lens distortion (include/sv_hip.h N3g): sv_lens_rays at 480 x 640 and 720 x 1280; decode_device and the cloud entry
         alone with and without a lens, registered and aligned; the packed stream's frames/s on lens frames.
No figure is a pass condition."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTIONS = ("decode", "host", "rgbd", "take", "lens")
LIMIT_S = {"decode": 240, "host": 240, "rgbd": 240, "take": 120, "lens": 240}
KINECT1_D = (0.159, -0.284, -0.003, 0.003, 0.0)  # plumb-bob, the size of the reference's Kinect 1 colour lens
RATIONAL_D = (5.6, 3.6, 3.2e-4, -1.1e-4, 0.18, 5.93, 5.44, 1.0)  # an Azure-Kinect-like depth lens
SCALE = 50


def make_frame(h, w, registered, filtered, seed=0, lens=False):
    """a wavy wall at 1.4 m with an end-effector blob at 0.8 m in the keyed colours of synth.gen_scene; the registered form has
    a depth camera of 0.8 times the colour camera's size, 1.2 degrees rotated and 20 mm to the side.  lens: the colour camera
    carries KINECT1_D and the depth camera of the registered form RATIONAL_D"""
    from mrcc_amd.utils.rgbd import RGBDFrame

    rng = np.random.default_rng(seed)
    hd, wd = (int(h * 0.8), int(w * 0.8)) if registered else (h, w)
    v, u = np.mgrid[0:hd, 0:wd]
    depth = 1400 + 60 * np.sin(u / (wd / 9.0) + seed) + 40 * np.cos(v / (hd / 7.0)) + rng.integers(-3, 4, size=(hd, wd))
    blob = (slice(int(hd * 0.3), int(hd * 0.63)), slice(int(wd * 0.35), int(wd * 0.6)))
    depth[blob] = 800 + 50 * np.sin(u[blob] / (wd / 27.0)) + 30 * np.cos(v[blob] / (hd / 24.0))
    depth = depth.astype(np.uint16)
    depth.reshape(-1)[rng.permutation(hd * wd)[: hd * wd // 1500]] = 0
    color = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    color[:, :, :2] = (color[:, :, :2] * 0.45).astype(np.uint8)
    ee = (slice(int(h * 0.3), int(h * 0.63)), slice(int(w * 0.35), int(w * 0.6)))
    color[ee[0], ee[1], 0] = rng.integers(205, 256, size=color[ee[0], ee[1], 0].shape)
    f = w * 0.875
    K = np.array([[f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]])
    kw = dict(filter_size=7 if filtered else 0, filter_thresh=300)
    if lens:
        kw.update(color_D=KINECT1_D, depth_D=RATIONAL_D if registered else KINECT1_D)
    if not registered:
        return RGBDFrame(depth, color, K, **kw)
    Kd = np.array([[0.74 * w, 0, (wd - 1) / 2], [0, 0.74 * w, (hd - 1) / 2], [0, 0, 1]])
    a = np.deg2rad(1.2)
    Hm = np.eye(4)
    Hm[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    Hm[:3, 3] = (0.02, 0.001, 0.0)
    return RGBDFrame(depth, color, Kd, K, Hm, **kw)


def fresh(frame):
    """the frame as a camera callback makes it: without its cached host registration and without its assembled byte buffer"""
    frame._registered = frame._buf = None
    return frame


def make_engine():
    import mrcc_amd
    from mrcc_amd.app.inference_engine import InferenceEngine
    from mrcc_amd.utils.config import Config

    Config.reset()
    Config().update({"INFERENCE": {"SEGMENTATION": {"scale": SCALE}}})
    eng = InferenceEngine(allow_random_init=True, seed=1)
    mrcc_amd.synth.wire_color_keyed_labels(eng._segmentation_model)
    return eng


def header():
    import torch

    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")


def decode():
    import torch

    from mrcc_amd.utils.packed import device_lut_values, normalized_color_table

    dev = torch.device("cuda")
    lut = torch.from_numpy(device_lut_values("float64")).to(dev)
    table = normalized_color_table("float64")
    header()
    for h, w in ((480, 640), (720, 1280)):
        for registered in (True, False):
            for filtered in (True, False):
                frame = make_frame(h, w, registered, filtered)
                t0 = time.perf_counter()
                for _ in range(3):
                    want = fresh(frame).decode_host(lut=table)
                host_ms = (time.perf_counter() - t0) / 3 * 1e3
                for _ in range(3):
                    got = fresh(frame).decode_device(dev, lut=lut)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    got = fresh(frame).decode_device(dev, lut=lut)
                torch.cuda.synchronize()
                dev_ms = (time.perf_counter() - t0) / 10 * 1e3
                assert np.array_equal(got[0].cpu().numpy().view(np.int32), want[0].view(np.int32))
                assert np.array_equal(got[2].cpu().numpy(), want[2])
                d_bytes = torch.from_numpy(frame._bytes()).to(dev)
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                for _ in range(20):
                    frame.unpack(d_bytes, lut=lut)
                end.record()
                torch.cuda.synchronize()
                print(f"decode:  {h} x {w} {'registered' if registered else 'aligned   '} filter {'7x7' if filtered else 'off'}: "
                      f"{len(want[2])} points; decode_host {host_ms:.1f} ms, decode_device {dev_ms:.3f} ms "
                      f"({host_ms / dev_ms:.0f} x), sv_rgbd_cloud alone {start.elapsed_time(end) / 20:.4f} ms per call "
                      f"(five launches and the wrapper's allocations, back to back)")


def frames_for_stream(count=4):
    return [make_frame(480, 640, registered=True, filtered=False, seed=s) for s in range(count)]


def host(frames, group):
    import torch

    from mrcc_amd.utils import preprocess

    eng, made = make_engine(), frames_for_stream()
    spent = [0.0]

    def decoded(n):
        for i in range(n):
            t0 = time.perf_counter()
            points, rgb, _ = fresh(made[i % len(made)]).decode_host(color="float64")
            rgb = preprocess.normalize_colors(rgb)
            spent[0] += time.perf_counter() - t0
            yield points, rgb

    for _ in range(2):
        labels = list(eng.predict_segmentation_stream(decoded(8), group=group))
    torch.cuda.synchronize()
    spent[0] = 0.0
    t0 = time.perf_counter()
    labels = list(eng.predict_segmentation_stream(decoded(frames), group=group))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    header()
    print(f"host:    decode_host + predict_segmentation_stream(group={group}), {frames} registered 480 x 640 frames of "
          f"{len(labels[0])} points: {frames / wall:.2f} frames/s, {wall / frames * 1e3:.3f} ms per frame, of which "
          f"{spent[0] / frames * 1e3:.3f} ms host decode (end-effector points in frame 0: {int((labels[0] == 2).sum())})")


def rgbd(frames, group):
    import torch

    eng, made = make_engine(), frames_for_stream()

    def items(n):
        for i in range(n):
            yield fresh(made[i % len(made)]), None, "float64"

    for _ in range(2):
        out = list(eng.predict_segmentation_stream(items(8), group=group))
    torch.cuda.synchronize()
    stream = next(iter(eng._seg_streams_packed.values()))
    stream.host_s.update({k: 0.0 for k in ("stage", "prepare", "launch", "finalize")})
    t0 = time.perf_counter()
    out = list(eng.predict_segmentation_stream(items(frames), group=group))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    header()
    print(f"rgbd:    packed stream(group={group}) on RGBDFrame items, {frames} registered 480 x 640 frames of {len(out[0][0])} "
          f"points: {frames / wall:.2f} frames/s, {wall / frames * 1e3:.3f} ms per frame, of which "
          f"{stream.host_s['stage'] / frames * 1e3:.3f} ms host stage (the images into one buffer, its copy to pinned memory, "
          f"upload, sv_rgbd_cloud launches, count read-back) (end-effector points in frame 0: {int((out[0][0] == 2).sum())})")


def lens(frames, group):
    import ctypes

    import torch

    from mrcc_amd._lib import call, ptr, stream_ptr
    from mrcc_amd.utils import rgbd as R
    from mrcc_amd.utils.packed import device_lut_values

    dev = torch.device("cuda")
    lut = torch.from_numpy(device_lut_values("float64")).to(dev)
    header()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for h, w in ((480, 640), (720, 1280)):
        f = w * 0.875
        table = torch.empty(h * w * 2 + 1, dtype=torch.float64, device=dev)
        cam4, dist = (ctypes.c_double * 4)(f, f, (w - 1) / 2, (h - 1) / 2), (ctypes.c_double * 8)(*RATIONAL_D)
        for timed in (False, True):
            torch.cuda.synchronize()
            start.record()
            for _ in range(10):
                call("sv_lens_rays", cam4, dist, h, w, ptr(table), stream_ptr())
            end.record()
            torch.cuda.synchronize()
        valid = int((table[:-1:2] == table[:-1:2]).sum().item())
        print(f"lens:    sv_lens_rays {h} x {w} (rational, 64 rounds): {start.elapsed_time(end) / 10:.4f} ms per call, "
              f"{valid} of {h * w} pixels valid, r2_max {float(table[-1].item()):.4f}")
    for h, w in ((480, 640), (720, 1280)):
        for registered in (True, False):
            for with_lens in (False, True):
                frame = make_frame(h, w, registered, filtered=False, lens=with_lens)
                for _ in range(3):  # the first call of a lens frame builds the camera's tables
                    got = fresh(frame).decode_device(dev, lut=lut)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    got = fresh(frame).decode_device(dev, lut=lut)
                torch.cuda.synchronize()
                dev_ms = (time.perf_counter() - t0) / 10 * 1e3
                want = frame.decode_host()
                assert np.array_equal(got[0].cpu().numpy().view(np.int32), want[0].view(np.int32))
                assert np.array_equal(got[2].cpu().numpy(), want[2])
                d_bytes = torch.from_numpy(frame._bytes()).to(dev)
                torch.cuda.synchronize()
                start.record()
                for _ in range(20):
                    frame.unpack(d_bytes, lut=lut)
                end.record()
                torch.cuda.synchronize()
                print(f"lens:    {h} x {w} {'registered' if registered else 'aligned   '} {'lens   ' if with_lens else 'pinhole'}: "
                      f"{len(want[2])} points; decode_device {dev_ms:.3f} ms, "
                      f"{'sv_rgbd_cloud_lens' if with_lens else 'sv_rgbd_cloud'} alone {start.elapsed_time(end) / 20:.4f} ms per call")
    eng = make_engine()
    made = [make_frame(480, 640, registered=True, filtered=False, seed=s, lens=True) for s in range(4)]

    def items(n):
        for i in range(n):
            yield fresh(made[i % len(made)]), None, "float64"

    for _ in range(2):
        out = list(eng.predict_segmentation_stream(items(8), group=group))
    torch.cuda.synchronize()
    builds = R.lens_table_builds
    t0 = time.perf_counter()
    out = list(eng.predict_segmentation_stream(items(frames), group=group))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(f"lens:    packed stream(group={group}) on RGBDFrame items with a lens, {frames} registered 480 x 640 frames of "
          f"{len(out[0][0])} points: {frames / wall:.2f} frames/s, {wall / frames * 1e3:.3f} ms per frame; tables built during "
          f"the timed run: {R.lens_table_builds - builds}")


def take():
    from mrcc_amd.utils.packed import normalized_color_table

    table = normalized_color_table("float64")
    for registered in (True, False):
        frame = make_frame(480, 640, registered, filtered=False)
        src = frame.decode_host()[2]
        crop = src[:: max(1, len(src) // 4096)][:4096]  # an end-effector crop's size
        times = []
        fresh(frame)
        for _ in range(4):
            t0 = time.perf_counter()
            frame.take(crop, lut=table)
            times.append((time.perf_counter() - t0) * 1e3)
        print(f"take:    480 x 640 {'registered' if registered else 'aligned'}, {len(crop)} pixels: first call {times[0]:.2f} ms"
              f"{' (runs the host registration)' if registered else ''}, later calls {min(times[1:]):.2f} ms")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--group", type=int, default=1)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child == "decode":
        return decode()
    if args.child == "host":
        return host(args.frames, args.group)
    if args.child == "rgbd":
        return rgbd(args.frames, args.group)
    if args.child == "take":
        return take()
    if args.child == "lens":
        return lens(args.frames, args.group)
    for section in args.sections.split(","):
        if section not in SECTIONS:
            raise SystemExit(f"unknown section {section!r}")
        subprocess.run(["timeout", "-k", "10", str(LIMIT_S[section]), sys.executable, os.path.abspath(__file__), "--child",
                        section, "--frames", str(args.frames), "--group", str(args.group)], check=True)


if __name__ == "__main__":
    main()
