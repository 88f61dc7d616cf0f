"""The device-image layer without a device: the voxel type every task of a list will see, the z-slab size, and
``device_image.Result`` on host data (``put`` and ``drain`` take anything with ``.cpu().numpy()``: a host tensor)."""
import numpy as np
import pytest

from magellanmapper_amd import config, device_image, transformer

torch = pytest.importorskip("torch")

K = config.PreProcessKeys
U16, F64 = np.dtype(np.uint16), np.dtype(np.float64)

# the expectations are the two rules the pre-checks of ``preprocess_img`` used to state apart -- ``denoise``: "float64
# if saturate or remap is ahead, else the image's"; ``rotate``: "float64 if anything is ahead" -- written out for a
# uint16 image.  The one place where they disagreed is a ``rotate`` behind a ``rotate``: the single statement says the
# image's type there (``rotate`` keeps it), where the old ``rotate`` rule said float64; the first ``rotate``'s check has
# then already passed or refused on the same settings, and float64 passes whatever uint16 passes.
TASK_LISTS = [
    ([], []),
    (["saturate"], [(K.SATURATE, U16)]),
    (["denoise"], [(K.DENOISE, U16)]),
    (["remap"], [(K.REMAP, U16)]),
    (["rotate"], [(K.ROTATE, U16)]),
    (["saturate", "denoise"], [(K.SATURATE, U16), (K.DENOISE, F64)]),
    (["rotate", "denoise"], [(K.ROTATE, U16), (K.DENOISE, U16)]),
    (["remap", "rotate"], [(K.REMAP, U16), (K.ROTATE, F64)]),
    (["rotate", "rotate"], [(K.ROTATE, U16), (K.ROTATE, U16)]),
    (["saturate", "sharpen", "rotate"], [(K.SATURATE, U16), (K.ROTATE, F64)]),
]


@pytest.mark.parametrize("names,want", TASK_LISTS, ids=[",".join(n) or "empty" for n, _ in TASK_LISTS])
def test_voxel_type_every_task_sees(names, want):
    assert transformer.tasks_ahead(names, np.uint16) == want


@pytest.mark.parametrize("n_chl", [1, 2])
@pytest.mark.parametrize("itemsize", [1, 2, 8])
def test_slab_step(monkeypatch, itemsize, n_chl):
    shape = (12, 16, 24) + ((n_chl,) if n_chl > 1 else ())
    plane = 16 * 24 * n_chl * itemsize
    monkeypatch.setattr(device_image, "SLAB_BYTES", 3 * plane)
    assert device_image.slab_step(shape, itemsize) == (3, 4)
    monkeypatch.setattr(device_image, "SLAB_BYTES", 5 * plane + plane - 1)
    assert device_image.slab_step(shape, itemsize) == (5, 3)
    monkeypatch.setattr(device_image, "SLAB_BYTES", 100 * plane)
    assert device_image.slab_step(shape, itemsize) == (12, 1)
    # a budget smaller than one plane: a plane at a time
    monkeypatch.setattr(device_image, "SLAB_BYTES", plane - 1)
    assert device_image.slab_step(shape, itemsize) == (1, 12)


def test_result_factory_is_called_once_with_the_final_shape_and_dtype(monkeypatch):
    made = []

    def factory(shape, dtype):
        made.append((shape, dtype))
        return np.full(shape, -1, dtype=dtype)
    src = torch.arange(12 * 4 * 5, dtype=torch.float64).reshape(12, 4, 5)
    monkeypatch.setattr(device_image, "SLAB_BYTES", 3 * 4 * 5 * 8)
    res = device_image.Result([12, 4, 5], "float64", out=factory)
    assert made == [((12, 4, 5), F64)]
    puts = []
    monkeypatch.setattr(device_image.Result, "put", lambda self, z0, z1, c, slab, _put=device_image.Result.put:
                        puts.append((z0, z1)) or _put(self, z0, z1, c, slab))
    res.drain(src)
    assert puts == [(0, 3), (3, 6), (6, 9), (9, 12)] and made == [((12, 4, 5), F64)]
    assert isinstance(res.value(), np.ndarray) and np.array_equal(res.value(), src.numpy())


def test_result_refuses_a_mismatching_out():
    for out in (np.empty((4, 5, 6), dtype=np.float32), np.empty((4, 5, 7), dtype=np.float64)):
        with pytest.raises(ValueError) as exc:
            device_image.Result((4, 5, 6), np.float64, out=out)
        assert str(exc.value) == f"out must be (4, 5, 6) float64, not {out.shape} {out.dtype}"
    out = np.empty((4, 5, 6), dtype=np.float64)
    assert device_image.Result((4, 5, 6), np.float64, out=out).value() is out


def test_result_zero_fill_and_a_channel_put():
    out = np.full((4, 3, 5, 2), 7, dtype=np.uint16)
    res = device_image.Result(out.shape, np.uint16, out=out, zero_fill=True)
    assert not out.any()
    slab = torch.full((2, 3, 5), 1.75, dtype=torch.float64)
    res.put(1, 3, 1, slab)
    want = np.zeros_like(out)
    want[1:3, ..., 1] = 1                   # (the assignment casts as NumPy's does)
    assert res.value() is out and np.array_equal(out, want)
    # without zero_fill the array given stays as it was wherever nothing is put
    keep = np.full((4, 3, 5), 7.0)
    res = device_image.Result(keep.shape, np.float64, out=keep)
    res.put(0, 2, None, slab)
    assert (keep[:2] == 1.75).all() and (keep[2:] == 7).all()
