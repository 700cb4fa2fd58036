"""Device-resident data provider, the parts that need no GPU: pld_batch_gather_flip's argument
checks (they return before any launch) and the opt-in switches of the public layers."""
import ctypes as C
import inspect

import pytest

from pldepth_amd import _lib
from pldepth_amd.data.providers.hourglass_provider import HourglassLargeScaleDataProvider

P = C.c_void_p(1 << 20)  # never dereferenced: every call below is rejected before a launch


def _call(imgs=P, gts=None, masks=None, n=5, h=3, w=4, c=3, idx=P, flip=None, B=2, x=P, gt=None,
          mask=None):
    return _lib.lib().pld_batch_gather_flip(imgs, gts, masks, n, h, w, c, idx, flip, B, x, gt,
                                            mask, None)


@pytest.mark.parametrize("bad", [
    dict(imgs=None), dict(idx=None), dict(x=None),           # required pointers
    dict(B=0), dict(n=0), dict(h=0), dict(w=-1), dict(c=0),  # non-positive sizes
    dict(gts=P), dict(gt=P), dict(masks=P), dict(mask=P),    # half-given pairs
    dict(B=1 << 20, h=1 << 10, w=1 << 10),                   # a batch of 2^40 pixels
])
def test_batch_gather_flip_rejects_bad_arguments(bad):
    with pytest.raises(_lib.PLDError, match="pld_batch_gather_flip"):
        _call(**bad)


def test_batch_gather_flip_signature_from_header():
    p, i = C.c_void_p, C.c_int
    assert _lib._SIGS["pld_batch_gather_flip"] == (i, [p, p, p, i, i, i, i, p, p, i, p, p, p, p])
    assert "pld_batch_gather_flip" not in _lib._NON_STATUS
    assert "hourglass_provider.py:29-62" in open(_lib.HEADER).read()


def test_device_data_click_option():
    from pldepth_amd.PLDepth import perform_pldepth_experiment
    opt = {p.name: p for p in perform_pldepth_experiment.params}["device_data"]
    assert opt.opts == ["--device_data"] and opt.default is False
    assert opt.type.name == "boolean"


def test_provider_device_resident_keyword():
    sig = inspect.signature(HourglassLargeScaleDataProvider.__init__)
    assert list(sig.parameters)[-1] == "device_resident"
    assert sig.parameters["device_resident"].default is False
