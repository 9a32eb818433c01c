"""sparse.layer_maps - the one table from a layer's shape to its kernel maps - for every layer shape the repository's
networks construct, and CoordinateManager.batches() with the batch count preset.  No GPU, no tensors."""
import pytest

from mrcc_amd.sparse import SAME_PLAN, CoordinateManager, CoordinateMap, LayerMaps, layer_maps

DOWN = LayerMaps(("down", "in"), (2, 1), ("up", "out"), False)


def strided(ks, st, dil=1):
    return LayerMaps(("strided", "in", ks, st, dil), (st, 1), ("strided_t", "in", ks, st, dil), False)


@pytest.mark.parametrize("shape,want", [
    # MinkUNet: conv0 / the blocks, the encoder's down convs, the decoder's transposed convs, `final` and the downsamples
    (dict(kernel_size=3, stride=1), LayerMaps(("k3", "in", 1), (1, 1), SAME_PLAN, True)),
    (dict(kernel_size=2, stride=2), DOWN),
    (dict(kernel_size=2, stride=2, transposed=True), LayerMaps(("up", "in"), (1, 2), ("down", "out"), False)),
    (dict(kernel_size=1, stride=1), LayerMaps(None, (1, 1), SAME_PLAN, False)),
    # the ResNets: the stem, conv5, a block's strided conv and its 1x1 downsample, dilated blocks
    (dict(kernel_size=3, stride=2), strided(3, 2)),
    (dict(kernel_size=3, stride=3), strided(3, 3)),
    (dict(kernel_size=1, stride=2), strided(1, 2)),
    (dict(kernel_size=3, stride=1, dilation=2), LayerMaps(("k3", "in", 2), (1, 1), SAME_PLAN, True)),
    (dict(kernel_size=3, stride=2, dilation=2), strided(3, 2, 2)),
    # local pooling (max, average and sum share the maps): the ResNet stem's k2 s2, k3 with and without a stride, k1
    (dict(kernel_size=2, stride=2, pooling=True), DOWN),
    (dict(kernel_size=3, stride=2, pooling=True), strided(3, 2)),
    (dict(kernel_size=3, stride=1, dilation=2, pooling=True),
     LayerMaps(("k3", "in", 2), (1, 1), ("strided_t", "in", 3, 1, 2), False)),
    (dict(kernel_size=1, stride=1, pooling=True), strided(1, 1)),
])
def test_layer_maps_rows(shape, want):
    assert layer_maps(**shape) == want


@pytest.mark.parametrize("shape,text", [
    (dict(kernel_size=5, stride=1), "kernel_size=5 stride=1 transposed=False: not used by the reference's U-Nets"),
    (dict(kernel_size=3, stride=2, transposed=True), "kernel_size=3 stride=2 transposed=True: not used by the reference's U-Nets"),
    (dict(kernel_size=3, stride=0), "kernel_size=3 stride=0 transposed=False: not used by the reference's U-Nets"),
    (dict(kernel_size=2, stride=1), "kernel_size=2 stride=1 transposed=False: not used by the reference's U-Nets"),
    (dict(kernel_size=5, stride=1, pooling=True), "pooling kernel_size=5 stride=1 dilation=1: no kernel map of that shape"),
    (dict(kernel_size=3, stride=0, pooling=True), "pooling kernel_size=3 stride=0 dilation=1: no kernel map of that shape"),
    (dict(kernel_size=2, stride=2, dilation=2, pooling=True),
     "pooling kernel_size=2 stride=2 dilation=2: no kernel map of that shape"),
])
def test_layer_maps_rejects_other_shapes(shape, text):
    with pytest.raises(NotImplementedError) as e:
        layer_maps(**shape)
    assert str(e.value) == text


class _Plans(CoordinateManager):
    """a manager whose plan_* methods record their calls instead of building anything"""

    def __init__(self):
        super().__init__("cpu")
        self.calls = []


def _recorder(name):
    def plan(self, *args):
        self.calls.append((name, *args))
        return (name, *args)
    return plan


for _name in ("plan_k3", "plan_down", "plan_up", "plan_strided", "plan_strided_t"):
    setattr(_Plans, _name, _recorder(_name))


def test_layer_plans_applies_a_row_lazily():
    cm = _Plans()
    plan, out, back, mirror = cm.layer_plans(layer_maps(2, 2), 4)
    assert (plan, out, mirror) == (("plan_down", 4), 8, False) and cm.calls == [("plan_down", 4)]
    assert back() == ("plan_up", 8) and cm.calls[-1] == ("plan_up", 8)  # built when asked for, from the output stride
    plan, out, back, mirror = cm.layer_plans(layer_maps(2, 2, transposed=True), 8)
    assert (plan, out, back()) == (("plan_up", 8), 4, ("plan_down", 4))
    plan, out, back, mirror = cm.layer_plans(layer_maps(3, 3, 2), 2)
    assert (plan, out, back()) == (("plan_strided", 2, 3, 3, 2), 6, ("plan_strided_t", 2, 3, 3, 2))
    n = len(cm.calls)
    plan, out, back, mirror = cm.layer_plans(layer_maps(3, 1), 2, plan="split")  # the caller's plan replaces the k3 map
    assert (plan, out, back(), mirror) == ("split", 2, "split", True) and len(cm.calls) == n
    assert cm.layer_plans(layer_maps(1, 1), 16)[:2] == (None, 16) and len(cm.calls) == n
    assert cm.layer_plans(layer_maps(3, 1, 2, pooling=True), 1)[2]() == ("plan_strided_t", 1, 3, 1, 2)


class _NoRead:
    def __getitem__(self, _):
        raise AssertionError("batches() read the coordinates although num_batches is set")


def test_batches_preset_reads_nothing():
    cm = CoordinateManager("cpu")
    cm.maps[1] = CoordinateMap(None, _NoRead(), 5, 1)
    cm.num_batches = 7
    assert cm.batches() == 7 and cm.num_batches == 7
