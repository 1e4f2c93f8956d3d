"""The long attention backward and the option that opens the image tower's training path to it, as far as no GPU is needed: the option's
default and environment name, the size query, the refusals that come before any launch, the unchanged Python refusal, the hazard scan."""
import os
import re
import shutil
import subprocess
import sys

import pytest

import vptfit_ref as ref
from clip_calibration_amd import _lib, maplefit, promptsrcfit, synthetic as syn, vptfit
from clip_calibration_amd.model import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_defaults_to_zero_and_round_trips():
    assert _lib.get_option("vision_train_long") == 0
    with _lib.option("vision_train_long", 1):
        assert _lib.get_option("vision_train_long") == 1 and vptfit.max_rows() == 640
    assert _lib.get_option("vision_train_long") == 0 and vptfit.max_rows() == 224 == vptfit.MAX_ROWS


@pytest.mark.parametrize("value", ("1", "0", ""))
def test_option_follows_the_environment(value):
    """The environment is read once per process: a fresh interpreter per value (this is what the test is about)."""
    code = "from clip_calibration_amd import _lib; print(_lib.get_option('vision_train_long'))"
    env = dict(os.environ, CLIPMI_VISION_TRAIN_LONG=value, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-1] == ("1" if value == "1" else "0")


def test_size_query_is_the_documented_formula():
    f = _lib.lib.clipmi_attention_backward_long_bytes
    for n, l, h in ((1, 1, 1), (2, 257, 2), (4, 259, 16), (64, 581, 1), (3, 640, 12)):
        assert f(n, l, h) == 12 * n * h * l
    assert f(1, 641, 1) == 0 and f(1, 0, 1) == 0 and f(0, 8, 1) == 0 and f(-1, 8, 1) == 0 and f(1, 8, 0) == 0
    assert f(1 << 30, 8, 2) == 0 and f(1 << 23, 640, 1) == 0


def test_refusals_need_no_gpu():
    f = _lib.lib.clipmi_attention_backward_long
    assert f(None, None, None, None, 0, 1, 641, 1, None) == _lib.ERR_SHAPE
    assert f(None, None, None, None, 0, 1, 0, 1, None) == _lib.ERR_SHAPE
    assert f(None, None, None, None, 0, -1, 8, 1, None) == _lib.ERR_SHAPE
    assert f(None, None, None, None, 0, 1, 8, 0, None) == _lib.ERR_SHAPE
    assert f(None, None, None, None, 0, 1, 640, 1, None) == _lib.ERR_ARG
    assert f(16, 16, 16, 8, 1 << 20, 1, 640, 1, None) == _lib.ERR_ARG          # a misaligned workspace
    assert f(16, 16, 16, 16, 12 * 640 - 1, 1, 640, 1, None) == _lib.ERR_ARG    # a short one
    assert f(None, None, None, None, 0, 0, 8, 1, None) == _lib.OK
    assert _lib.lib.clipmi_attention_backward_full(None, None, None, 1, 225, 1, None) == _lib.ERR_SHAPE


def test_python_refusal_text_at_option_zero_is_unchanged():
    assert _lib.get_option("vision_train_long") == 0
    big = build_model(dict(syn.synthetic_state_dict(ref.CUSTOM, seed=0)),
                      {"trainer": "VPT", "vision_depth": 1, "vision_ctx": 28, "language_depth": 0, "language_ctx": 0})
    with pytest.raises(ValueError) as e:
        vptfit._check_prompts("VPTFitState", big, vptfit.model_prompts(big))
    assert str(e.value) == "VPTFitState: 197 tokens + 28 prompt rows = 225 rows per image; the backward takes at most 224"
    with pytest.raises(ValueError) as e:
        vptfit.check_rows("MaPLeFitState", 257, 2)
    assert str(e.value) == "MaPLeFitState: 257 tokens + 2 prompt rows = 259 rows per image; the backward takes at most 224"
    with _lib.option("vision_train_long", 1):
        vptfit.check_rows("MaPLeFitState", 257, 2)
        vptfit.check_rows("PromptSRCFitState", 577, 63)
        with pytest.raises(ValueError, match="at most 640"):
            vptfit.check_rows("PromptSRCFitState", 577, 64)
        assert tuple(vptfit._check_prompts("VPTFitState", big, vptfit.model_prompts(big))) == (1, 28)
    assert maplefit.vptfit is vptfit and promptsrcfit.vptfit is vptfit          # one limit for the three fits


def test_package_surface():
    for name in ("clipmi_attention_backward_long", "clipmi_attention_backward_long_bytes"):
        assert hasattr(_lib.lib, name), name
    from clip_calibration_amd import ops
    assert callable(ops.attention_backward_long) and callable(vptfit.stash_bytes) and callable(vptfit.max_rows)
    header = open(os.path.join(ROOT, "include", "clipmi.h")).read()
    for word in ("clipmi_attention_backward_long_bytes", "clipmi_attention_backward_long(", "vision_train_long", "CLIPMI_VISION_TRAIN_LONG"):
        assert word in header, word


def test_hazard_scan_reports_nothing_on_the_attention_translation_unit():
    """tools/mfma_hazard_scan.py over attention.hip, called as tests/test_cabi_cpu.py calls it: no VALU-written MFMA source closer than four
    wait states, with the two new kernels among the kernels walked."""
    if shutil.which(os.environ.get("HIPCC", "hipcc")) is None:
        pytest.skip("no hipcc on this box: the ISA cannot be produced")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mfma_hazard_scan.py"), "attention.hip"],
                       env=dict(os.environ, WAIT="4"), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"attention\.hip: 0 VALU write -> MFMA source sites .* \((\d+) MFMA kernels, (\d+) MFMA instructions walked\)", r.stdout)
    assert m and int(m.group(1)) >= 14 and int(m.group(2)) >= 32, r.stdout[-2000:]      # twelve kernels before this pair
