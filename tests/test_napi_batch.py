"""Parallel.msmBatch of the JS facade against Parallel.msm on the golden vectors (js/test-batch.js).  `-m gpu`."""
import pytest

from napi_support import run_js


@pytest.mark.gpu
def test_js_msm_batch_equals_msm():
    run_js("test-batch.js", 600)
