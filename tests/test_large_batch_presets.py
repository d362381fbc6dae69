"""The large-batch presets: they exist, validate, differ from `mspacman` in
the batch size alone, and sit after the presets pinned by
test_reference_preset.py."""

import pytest

from r2d2_amd import config as cfg

PINNED = ["cartpole", "mspacman", "mspacman_gpu_replay", "mspacman_dp",
          "seaquest_impala", "mspacman_reference",
          "mspacman_reference_gpu_replay"]


def test_large_batch_presets_come_after_the_pinned_ones():
    names = list(cfg.PRESETS)
    assert names[:len(PINNED)] == PINNED
    assert names[len(PINNED):len(PINNED) + 2] == ["mspacman_b128",
                                                  "mspacman_b256"]


@pytest.mark.parametrize("name,batch", [("mspacman_b128", 128),
                                        ("mspacman_b256", 256)])
def test_large_batch_preset_is_mspacman_with_a_batch_size(name, batch):
    base = cfg.apply("mspacman")
    c = cfg.apply(name)
    assert c.batch_size == batch and cfg.batch_size == batch
    diff = {k for k in cfg.Config.__dataclass_fields__
            if getattr(c, k) != getattr(base, k)}
    assert diff == {"batch_size"}, diff
    assert c.encoder == "nature" and c.hidden_dim == 512
    assert c.use_hip_kernels and not c.gpu_replay
    # field overrides still apply on top of the preset
    assert cfg.apply(name, batch_size=96).batch_size == 96


def test_engine_batch_limit_is_256():
    from r2d2_amd.ops.engine import MAX_BATCH_SIZE, check_batch_size
    assert MAX_BATCH_SIZE == 256
    check_batch_size(1)
    check_batch_size(256)
    for bad in (0, 257, 1024):
        with pytest.raises(ValueError, match="batch_size <= 256"):
            check_batch_size(bad)
