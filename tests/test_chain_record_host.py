"""The chain recorder's host side (no GPU): the record schedule, its timestep mapping, the argument refusals of the new C
entries and the Python refusals that need no device."""
import ctypes as C

import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi
from cindm_amd import dist as cdist
from cindm_amd.record import ChainRecord, LoopRecorder, record_schedule, record_times, stream_mask


def _expected_steps(n, every):
    """The issue's rule, spelled out: the state after step i (0-based) is recorded iff (i + 1) % every == 0 or i == n - 1."""
    return [i + 1 for i in range(n) if (i + 1) % every == 0 or i == n - 1]


@pytest.mark.parametrize("n", [1, 12, 13])
@pytest.mark.parametrize("every", [1, 4, 13, 50])
def test_record_schedule(n, every):
    steps = record_schedule(n, every)
    assert steps == _expected_steps(n, every)
    assert len(steps) == -(-n // every) and steps[-1] == n          # ceil(n / every) records, the last one is the result
    assert steps == sorted(set(steps)) and steps[0] >= 1


def test_record_schedule_named_cases():
    assert record_schedule(13, 4) == [4, 8, 12, 13]
    assert record_schedule(12, 4) == [4, 8, 12]
    assert record_schedule(10, 3) == [3, 6, 9, 10]
    assert record_schedule(4, 3) == [3, 4]
    assert record_schedule(5, 50) == [5]
    # "only the result": an every at the top of int32 on chains of two or more steps
    assert record_schedule(2, 2 ** 31 - 1) == [2] and record_schedule(13, 2 ** 31 - 1) == [13]
    assert record_times(record_schedule(13, 2 ** 31 - 1), t_start=999) == [987]
    for bad in ((0, 1), (5, 0), (5, -2)):
        with pytest.raises(ValueError):
            record_schedule(*bad)


def test_record_times():
    # DDPM: step i runs timestep t_start - i
    assert record_times([4, 8, 12, 13], t_start=999) == [996, 992, 988, 987]
    assert record_times([1], t_start=0) == [0]
    # DDIM: step i runs times[i]; the closing -1 of the schedule is never a step's own timestep
    times = [999, 899, 799, 699, 599, 499, 399, 299, 199, 99, -1]
    assert record_times(record_schedule(10, 3), times=times) == [799, 499, 199, 99]
    assert record_times(record_schedule(10, 1), times=times) == times[:-1]
    with pytest.raises(ValueError):
        record_times([1], t_start=5, times=times)
    with pytest.raises(ValueError):
        record_times([1])


def test_stream_mask():
    assert stream_mask(("x",)) == 1 and stream_mask(("x", "x0")) == 3 and stream_mask("x0") == 2 and stream_mask(["x0", "x"]) == 3
    with pytest.raises(ValueError):
        stream_mask(("x", "eps"))
    with pytest.raises(ValueError):
        stream_mask(())


def test_loop_recorder_follows_the_schedule():
    """The Python-loop routes clone per step with the same indexing as the device recorder."""
    r = LoopRecorder(5, 2, ("x", "x0"), t_start=999)
    for i in range(5):
        r.after(i, torch.full((2, 3), float(i)), torch.full((2, 3), 10.0 + i))
    rec = r.result()
    assert isinstance(rec, ChainRecord) and cindm_amd.ChainRecord is ChainRecord
    assert rec.step == [2, 4, 5] and rec.t == [998, 996, 995] and len(rec) == 3
    assert rec.x.shape == (3, 2, 3) and [float(v) for v in rec.x[:, 0, 0]] == [1.0, 3.0, 4.0]
    assert [float(v) for v in rec.x0[:, 0, 0]] == [11.0, 13.0, 14.0]
    r.reset()
    r.after(0, torch.zeros(1))
    assert r.result().x is None                      # step 1 is not on the schedule


def test_c_entries_refuse_bad_arguments():
    L = _ffi.lib()
    raw = (C.c_char * 80)()                          # never dereferenced: every call below is refused on its arguments
    aligned = C.c_void_p((C.addressof(raw) + 15) & ~15)
    assert L.cindm_ddpm1d_set_recorder(None, aligned, 4, 1, 1) != 0
    assert b"null handle" in L.cindm_last_error()
    assert L.cindm_ddpm1d_set_recorder(None, aligned, 4, 0, 1) != 0
    assert b"every" in L.cindm_last_error()
    assert L.cindm_ddpm1d_set_recorder(None, aligned, 4, 1, 4) != 0
    assert b"stream" in L.cindm_last_error()
    assert L.cindm_ddpm1d_set_recorder(None, aligned, 4, 1, 0) != 0
    assert b"stream" in L.cindm_last_error()
    assert L.cindm_ddpm1d_set_recorder(None, None, 0, 1, 1) != 0          # disarming needs a handle too
    assert b"null handle" in L.cindm_last_error()
    info = (C.c_int32 * 4)()
    assert L.cindm_ddpm1d_recorder_info(None, info) != 0
    assert b"null" in L.cindm_last_error()


class _Refuses:
    """A diffusion whose sample methods must never be reached."""

    def sample(self, **kw):
        raise AssertionError("the sharded helper called sample()")

    def sample_compose_multibodies(self, *a, **kw):
        raise AssertionError("the sharded helper called sample_compose_multibodies()")


def test_sharded_helpers_reject_the_keyword():
    d = _Refuses()
    with pytest.raises(ValueError, match="chain records"):
        cdist.sample_sharded(d, 4, seed=1, return_trajectory_every=2)
    with pytest.raises(ValueError, match="chain records"):
        cdist.sample_sharded(d, 4, seed=1, trajectory=("x", "x0"))
    with pytest.raises(ValueError, match="chain records"):
        cdist.sample_multibodies_sharded(d, torch.zeros((4, 4, 16)), 400, 0, 4, seed=1, return_trajectory_every=2)
    with pytest.raises(ValueError, match="chain records"):
        cdist.sample2d_sharded(d, 4, seed=1, num_boundaries=2, return_trajectory_every=2)


def _diffusion2d(**kw):
    sd = O.synth_state_dict_2d(O.unet2d_param_shapes(64, (1, 2), 21), 0)
    m = cindm_amd.Unet(dim=64, dim_mults=(1, 2), channels=21)
    m.load_state_dict(sd, strict=True)
    return cindm_amd.GaussianDiffusion(m, image_size=64, frames=6, timesteps=1000, **kw)


def test_2d_refusals_that_need_no_device():
    d = _diffusion2d(sampling_timesteps=50)
    with pytest.raises(NotImplementedError, match="return_all_timesteps"):
        d.sample(batch_size=1, num_boundaries=2, return_all_timesteps=True)
    with pytest.raises(NotImplementedError, match="return_all_timesteps"):
        d.sample(batch_size=1, num_boundaries=2, return_all_timesteps=True, return_trajectory_every=2)
    with pytest.raises(NotImplementedError, match="x0"):
        d.sample(batch_size=1, num_boundaries=2, return_trajectory_every=2, trajectory=("x", "x0"))
    with pytest.raises(ValueError, match="stream"):
        d.sample(batch_size=1, num_boundaries=2, return_trajectory_every=2, trajectory=("eps",))


def test_1d_refusals_that_need_no_device():
    sd = O.synth_state_dict(O.unet1d_param_shapes(24, 8, attention=True), seed=0)
    m = cindm_amd.TemporalUnet1D(24, 8, False, attention=True)
    m.load_state_dict(sd, strict=True)
    d = cindm_amd.GaussianDiffusion1D(m, image_size=20, conditioned_steps=4, sampling_timesteps=10)
    with pytest.raises(NotImplementedError, match="return_trajectory_every"):
        d.autoregress_time_compose_sample(2, torch.zeros((2, 4, 8)), 1, return_trajectory_every=2)
    with pytest.raises(NotImplementedError, match="return_trajectory_every"):
        d.sample_compose_multibodies(torch.zeros((2, 4, 16)), 1000, 3, 4, return_trajectory_every=2)
