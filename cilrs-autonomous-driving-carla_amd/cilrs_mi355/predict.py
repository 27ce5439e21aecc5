"""Inference adapter -- counterpart of AutonomousDriver.preprocess_image / predict_controls
(reference model/autonomous_drive.py:481-485, 897-920).

Frames at the network resolution (88x200) take the uint8 path: /255, HWC->CHW and
Normalize(mean, std) fused into one HIP kernel that writes the NHWC tensor the stem reads.  Frames
of any other size (the agent's camera is 800x600, 4 bytes per pixel, :868-872) take the camera
path, which also fuses the reference's host-side cv2.resize (8-bit INTER_LINEAR, restated from
OpenCV's published fixed-point algorithm -- cv2 is not in the build image, so that step is
parity-unpinned) into the same kernel: the whole of preprocess_image runs on the device.
"""
from __future__ import annotations

import ctypes as _C
import os

import numpy as np
import torch

from . import _lib as _L

IMG_MEAN = (0.485, 0.456, 0.406)       # autonomous_drive.py:481
IMG_STD = (0.229, 0.224, 0.225)        # :482
IMG_WIDTH, IMG_HEIGHT = 200, 88        # :483-484
SPEED_NORM_FACTOR = 90.0               # :485


class _FastTick:
    """Everything one persistent tick hands to the library, bound once per weight epoch."""
    __slots__ = ("sync_fn", "post_fn", "handle", "bufs", "frame", "speed", "cmd", "ctrl", "spd",
                 "stream", "plan", "done")


# ticks served through the per-layer launches after a barrier timeout before the persistent launch
# is tried again (10 s of a 20 Hz control loop)
DEGRADED_TICKS = 200
# what the library says when the persistent launch's planner has no tiling for a frame size (it
# needs every stage in one pass of the resident grid); said before anything is launched
PLANNER_REFUSALS = ("no one-pass tiling", "frame too large for", "division constants do not cover")


class Predictor:
    """Holds pinned staging buffers so a 20 Hz control loop does one H2D and one D2H copy per
    tick (the reference does four ``.item()`` syncs, :918-920).  ``use_graph=True`` replays the
    forward from a cached hipGraph; measured on MI355X the eager launch sequence is as fast
    (0.48 ms end to end at B=1 either way: the path is bound by ~60 dependent small kernels, not
    by host launch overhead), so it is off by default.  A command outside 0..3 raises, like the
    reference's torch.gather (the status word rides along with the output copy)."""

    def __init__(self, model, batch=1, height=IMG_HEIGHT, width=IMG_WIDTH, use_graph=False,
                 half=False, persistent=None):
        self.model = model.eval()
        self.eng = model.engine()
        dev = self.eng.device
        self.batch = batch
        self.use_graph = use_graph
        self.half = half              # fp16 BasicBlock trunk (batched serving, BASELINE config 5)
        # one fp32 frame of the reference network: the whole forward as ONE persistent launch
        # (csrc/infer_b1.hip) -- the default of the single-frame control loop
        if persistent is None:
            persistent = batch == 1 and not half and self.eng.variant == 0
        self.persistent = bool(persistent)
        self.stream = torch.cuda.Stream(device=dev)      # hipGraph capture needs its own stream
        # ONE pinned host buffer and ONE device buffer per direction: a tick costs one H2D copy
        # (frames | speed | command, packed) and one D2H copy (controls | predicted speed)
        nfr = batch * height * width * 3
        o_spd = (nfr + 15) // 16 * 16
        o_cmd = (o_spd + 4 * batch + 7) // 8 * 8
        self.in_host = torch.zeros(o_cmd + 8 * batch, dtype=torch.uint8).pin_memory()
        self.in_dev = torch.zeros_like(self.in_host, device=dev)

        def views(buf):
            return (buf[:nfr].view(batch, height, width, 3),
                    buf[o_spd:o_spd + 4 * batch].view(torch.float32),
                    buf[o_cmd:o_cmd + 8 * batch].view(torch.int64))
        self.frames_host, self.speed_host, self.cmd_host = views(self.in_host)
        self.frames_dev, self.speed_dev, self.cmd_dev = views(self.in_dev)
        self.out_dev = torch.empty(batch * 4, dtype=torch.float32, device=dev)
        # [controls | predicted speed | completion word of the persistent launch]
        self.out_host = torch.zeros(batch * 4 + 4, dtype=torch.float32).pin_memory()
        self.ctrl_dev = self.out_dev[:batch * 3].view(batch, 3)
        self.spd_out_dev = self.out_dev[batch * 3:]
        self._ctrl_host = self.out_host[:batch * 3].view(batch, 3)
        self._spd_host = self.out_host[batch * 3:batch * 4]
        self._done_host = self.out_host[batch * 4:batch * 4 + 1].view(torch.int32)
        self._done_np = self._done_host.numpy()
        self._seq = 0
        # CILRS_B1_SPIN=0: wait with hipStreamSynchronize instead of spinning on the completion word
        self.spin = os.environ.get("CILRS_B1_SPIN", "1") != "0"
        # CILRS_B1_ZERO_COPY=0: stage through device buffers (A/B switch of tools/infer_b1_probe.py)
        self.zero_copy = os.environ.get("CILRS_B1_ZERO_COPY", "1") != "0"
        self._ctrl_np = self.out_host[:batch * 3].view(batch, 3).numpy()
        self._spd_np = self.out_host[batch * 3:batch * 4].numpy()
        self._frames_np = self.frames_host.numpy()
        self._speed_np = self.speed_host.numpy()
        self._cmd_np = self.cmd_host.numpy()
        self._seen_epoch = -1
        self._fast = None
        # degraded mode of the persistent launch (see _barrier_gave_up)
        self.degraded_ticks_left = 0
        self.barrier_timeouts = 0
        self._warned_degraded = False
        self._inject_timeout = 0      # tests: simulate this many barrier timeouts

    def _order_after_weight_updates(self):
        # The forward runs on this predictor's own stream.  Whatever last wrote the weights (a
        # train step, load_state_dict, an optimiser) was enqueued on the caller's current stream:
        # order this stream behind it -- only when the engine's weight epoch moved, so the
        # steady-state control loop pays nothing.
        if self._seen_epoch != self.eng.weights_epoch:
            self.stream.wait_stream(torch.cuda.current_stream(self.eng.device))
            self._seen_epoch = self.eng.weights_epoch

    def _check_commands(self, commands):
        # the command comes from the host (route planner, autonomous_drive.py:1589-1593): validate
        # it here -- a value outside 0..num_commands-1 raises exactly where the reference's torch.gather does
        # (:397-398, :915-917), without waiting for the device's status word
        c = np.asarray(commands, dtype=np.int64)
        nc = getattr(self.model, "num_commands", 4)
        if c.size and (c.min() < 0 or c.max() >= nc):
            raise RuntimeError(f"predict_controls: command index out of range (expected 0..{nc - 1})")
        return c

    @staticmethod
    def _result4(controls, pred_speed):
        """np.float32 [B,4] = (steer, throttle, brake, speed_kmh) from the pinned outputs of a
        forward: controls [B,3] (or flat) and the normalised pred_speed [B]."""
        out = np.empty((pred_speed.shape[0], 4), dtype=np.float32)
        out[:, :3] = controls.reshape(-1, 3)
        out[:, 3] = pred_speed * np.float32(SPEED_NORM_FACTOR)                  # :920
        return out

    @torch.no_grad()
    def predict_batch(self, frames_u8, speeds_kmh, commands):
        """frames uint8 [B,88,200,3] RGB, km/h, command idx -> np.float32 [B,4] =
        (steer, throttle, brake, speed_kmh)."""
        if self.model.engine() is not self.eng:
            self.__init__(self.model, self.batch, self.frames_host.size(1),
                          self.frames_host.size(2), self.use_graph, self.half, self.persistent)
        if self.model.training:
            self.model.eval()
        if self.persistent and self.zero_copy:
            return self._tick_persistent(frames_u8, speeds_kmh, commands)
        # host staging through NUMPY views of the pinned buffers: torch CPU ops would wake the
        # intra-op thread pool, whose spinning workers exhaust a container's CPU quota and stall
        # the control loop for ~90 ms every ~200 ms (measured: tools/stall_probe2.py)
        np.copyto(self._frames_np, np.asarray(frames_u8, dtype=np.uint8))
        # min(speed_kmh / 90.0, 1.0) in double like the reference (:910), then float32
        self._speed_np[...] = np.minimum(
            np.asarray(speeds_kmh, dtype=np.float64) / SPEED_NORM_FACTOR, 1.0)
        np.copyto(self._cmd_np, self._check_commands(commands))
        self._order_after_weight_updates()
        with torch.cuda.stream(self.stream):
            if self.persistent and self.zero_copy:
                # the one launch reads the frame / speed / command straight from the pinned
                # staging buffer and writes its four outputs into pinned host memory: no copy
                # commands on the stream, one launch + one synchronisation per tick
                self.eng.run_forward_u8(self.frames_host, self.speed_host, self.cmd_host,
                                        out=(self._ctrl_host, self._spd_host), persistent=True)
                self.stream.synchronize()
            else:
                self.in_dev.copy_(self.in_host, non_blocking=True)
                try:
                    self.eng.run_forward_u8(self.frames_dev, self.speed_dev, self.cmd_dev,
                                            out=(self.ctrl_dev, self.spd_out_dev),
                                            graph=self.use_graph, half=self.half,
                                            persistent=self.persistent)
                except RuntimeError:
                    if not (self.persistent and self._planner_refused()):
                        raise
                    self.eng.run_forward_u8(self.frames_dev, self.speed_dev, self.cmd_dev,
                                            out=(self.ctrl_dev, self.spd_out_dev),
                                            graph=self.use_graph, half=self.half, persistent=False)
                self.out_host[:self.batch * 4].copy_(self.out_dev, non_blocking=True)   # pinned; no torch kernels
                self.stream.synchronize()
        if self.persistent and not np.isfinite(self._ctrl_np).all():
            self.eng.check_status()       # a grid barrier that gave up leaves NaN outputs
        return self._result4(self._ctrl_np, self._spd_np)

    def _tick_persistent(self, frames_u8, speeds_kmh, commands):
        """One control-loop tick on the persistent launch: stage the inputs in the pinned buffer
        (numpy), ONE library call that launches and synchronises, read the pinned outputs.  The
        kernel reads the frame and writes its four floats in host memory itself."""
        np.copyto(self._frames_np, frames_u8, casting="unsafe")
        self._speed_np[...] = np.minimum(
            np.asarray(speeds_kmh, dtype=np.float64) / SPEED_NORM_FACTOR, 1.0)
        np.copyto(self._cmd_np, self._check_commands(commands))
        eng = self.eng
        if self.degraded_ticks_left > 0:
            self.degraded_ticks_left -= 1
            return self._tick_per_layer()
        fast = self._fast
        if fast is None or self._seen_epoch != eng.weights_epoch:
            self._order_after_weight_updates()
            pl = eng.plan(self.batch, self.frames_host.size(1), self.frames_host.size(2))
            eng._announce_weights(pl)
            eng.last_plan = pl
            L = _L
            fast = self._fast = _FastTick()
            fast.sync_fn = L.lib().cilrs_net_forward_u8_b1_sync
            fast.post_fn = L.lib().cilrs_net_forward_u8_b1_post
            fast.handle, fast.bufs, fast.plan = pl.handle, _C.byref(pl.bufs), pl
            fast.frame, fast.speed, fast.cmd = (L.ptr(self.frames_host), L.ptr(self.speed_host),
                                                L.ptr(self.cmd_host))
            fast.ctrl, fast.spd = L.ptr(self._ctrl_host), L.ptr(self._spd_host)
            fast.stream = _C.c_void_p(self.stream.cuda_stream)
            fast.done = L.ptr(self._done_host)
        if self.spin:
            # the launch posts its own completion word behind the outputs: spin on it instead of
            # waiting for the stream's completion signal
            self._seq = seq = (self._seq % 0x3FFFFFFF) + 1
            if fast.post_fn(fast.handle, fast.bufs, fast.frame, fast.speed, fast.cmd, fast.ctrl,
                            fast.spd, fast.done, seq, fast.stream) != 0:
                if self._planner_refused():
                    return self._tick_per_layer()
                _L.check(1)
            done, n = self._done_np, 0
            while done[0] != seq:
                n += 1
                if n > 2000000:             # ~seconds: something is wrong; let the stream tell us
                    self.stream.synchronize()
                    break
        elif fast.sync_fn(fast.handle, fast.bufs, fast.frame, fast.speed, fast.cmd, fast.ctrl,
                          fast.spd, fast.stream) != 0:
            if self._planner_refused():
                return self._tick_per_layer()
            _L.check(1)
        if self._inject_timeout > 0:      # test hook: what the kernel leaves behind on a timeout
            self._inject_timeout -= 1
            self.stream.synchronize()
            fast.plan.status[1] = 1
            self._ctrl_np[...] = np.nan
            self._spd_np[...] = np.nan
        if not np.isfinite(self._ctrl_np).all() and self._barrier_gave_up(fast.plan):
            return self._tick_per_layer()
        return self._result4(self._ctrl_np, self._spd_np)

    def _planner_refused(self):
        """A persistent call just failed.  If the library's planner said that it has no tiling
        for this frame size (nothing was launched, the status words are untouched), that is
        not an error of the frame either: this predictor serves every tick through the per-layer
        launches from now on, reports ``persistent`` False, and says so once."""
        msg = _L.lib().cilrs_last_error()
        msg = msg.decode() if msg else ""
        if not any(r in msg for r in PLANNER_REFUSALS):
            return False
        self.persistent = False
        self._fast = None
        import warnings
        warnings.warn("CILRS Predictor: the persistent single-frame launch does not serve "
                      f"{self.frames_host.size(1)}x{self.frames_host.size(2)} frames ({msg}); "
                      "serving them through per-layer launches", RuntimeWarning)
        return True

    def _barrier_gave_up(self, plan):
        """Non-finite outputs of the persistent launch.  If its status word says a grid barrier
        gave up (another resident kernel held CUs: the launch cannot make progress while it is
        not fully resident), this is not an error of the frame: the reference's control loop never
        raises mid-drive (model/autonomous_drive.py:908-920), so the tick is served through the
        per-layer launches in the same process, the next DEGRADED_TICKS ticks too, and a warning is
        printed once.  Anything else (a bad command, NaN weights) goes through check_status."""
        bad_cmd, barrier = plan.take_status()
        if not barrier:
            if bad_cmd:
                plan.status[0] = 1
                self.eng.check_status()
            return False
        if bad_cmd:
            plan.status[0] = 1            # keep the other finding for the next check
        self.barrier_timeouts += 1
        self.degraded_ticks_left = DEGRADED_TICKS
        if not self._warned_degraded:
            self._warned_degraded = True
            import warnings
            warnings.warn("CILRS Predictor: a grid barrier of the persistent single-frame launch gave "
                          "up (another kernel was resident on the device); serving this and the next "
                          f"{DEGRADED_TICKS} ticks through per-layer launches", RuntimeWarning)
        return True

    def _tick_per_layer(self):
        """The staged inputs through the per-layer launch path (device staging buffers)."""
        self._order_after_weight_updates()
        with torch.cuda.stream(self.stream):
            self.in_dev.copy_(self.in_host, non_blocking=True)
            self.eng.run_forward_u8(self.frames_dev, self.speed_dev, self.cmd_dev,
                                    out=(self.ctrl_dev, self.spd_out_dev), graph=self.use_graph,
                                    half=self.half, persistent=False)
            self.out_host[:self.batch * 4].copy_(self.out_dev, non_blocking=True)
            self.stream.synchronize()
        return self._result4(self._ctrl_np, self._spd_np)

    @torch.no_grad()
    def predict_camera(self, frame_u8, speed_kmh, command_idx):
        """One raw camera frame uint8 [Hs,Ws,3|4] -> (steer, throttle, brake, speed_kmh); the
        resize happens on the device (preprocess_image, :897-902)."""
        if self.batch != 1:
            raise RuntimeError("predict_camera is the single-frame control-loop path")
        frame = np.asarray(frame_u8, dtype=np.uint8)
        if frame.ndim != 3 or frame.shape[2] not in (3, 4):
            raise RuntimeError("camera frame must be uint8 [Hs,Ws,3 or 4]")
        if self.model.engine() is not self.eng:
            self.__init__(self.model, self.batch, self.frames_host.size(1),
                          self.frames_host.size(2), self.use_graph, self.half, self.persistent)
        if self.model.training:
            self.model.eval()
        cam = getattr(self, "_cam", None)
        if cam is None or cam[3] != frame.shape:
            nfr = frame.size
            o_spd = (nfr + 15) // 16 * 16
            host = torch.zeros(o_spd + 16, dtype=torch.uint8).pin_memory()
            dev = torch.zeros_like(host, device=self.eng.device)

            def views(buf):
                return (buf[:nfr].view((1,) + frame.shape), buf[o_spd:o_spd + 4].view(torch.float32),
                        buf[o_spd + 8:o_spd + 16].view(torch.int64))
            hv, dv = views(host), views(dev)
            cam = (host, (hv[0].numpy(), hv[1].numpy(), hv[2].numpy()), (dev,) + dv, frame.shape,
                   (hv[1], hv[2]))
            self._cam = cam
        np.copyto(cam[1][0][0], frame)
        cam[1][1][...] = min(float(speed_kmh) / SPEED_NORM_FACTOR, 1.0)
        cam[1][2][...] = self._check_commands([int(command_idx)])
        if self.persistent and self.zero_copy and self.degraded_ticks_left > 0:
            self.degraded_ticks_left -= 1
        elif self.persistent and self.zero_copy:
            # the transform kernel samples the pinned camera frame in place (it touches a fraction
            # of its 1.9 MB), the persistent launch starts at its second stage; one library call
            eng = self.eng
            if self._seen_epoch != eng.weights_epoch or self._fast is None:
                self._order_after_weight_updates()
                pl = eng.plan(1, self.frames_host.size(1), self.frames_host.size(2))
                eng._announce_weights(pl)
                self._fast = None
            pl = eng.plan(1, self.frames_host.size(1), self.frames_host.size(2))
            eng.last_plan = pl
            hs, ws_, px = frame.shape
            refused = False
            if _L.lib().cilrs_net_forward_camera_b1(
                    pl.handle, _C.byref(pl.bufs), _L.ptr(cam[0]), hs, ws_, px, ws_ * px,
                    _L.ptr(cam[4][0]), _L.ptr(cam[4][1]), _L.ptr(self._ctrl_host),
                    _L.ptr(self._spd_host), 1, _C.c_void_p(self.stream.cuda_stream)) != 0:
                refused = self._planner_refused()
                if not refused:
                    _L.check(1)
            if not refused and (np.isfinite(self._ctrl_np).all() or not self._barrier_gave_up(pl)):
                c = self._ctrl_np[0]
                return (float(c[0]), float(c[1]), float(c[2]),
                        float(self._spd_np[0]) * SPEED_NORM_FACTOR)
            # (barrier timeout, or no tiling for this size: the per-layer camera path below)
        self._order_after_weight_updates()
        with torch.cuda.stream(self.stream):
            cam[2][0].copy_(cam[0], non_blocking=True)               # frame | speed | command
            self.eng.run_forward_camera(cam[2][1], cam[2][2], cam[2][3],
                                        self.frames_host.size(1), self.frames_host.size(2),
                                        out=(self.ctrl_dev, self.spd_out_dev))
            self.out_host[:self.batch * 4].copy_(self.out_dev, non_blocking=True)
            self.stream.synchronize()
        c = self._ctrl_np[0]
        return (float(c[0]), float(c[1]), float(c[2]), float(self._spd_np[0]) * SPEED_NORM_FACTOR)

    # ---- saliency ----------------------------------------------------------------------------
    SALIENCY_OUTPUTS = {"steer": (1.0, 0.0, 0.0, 0.0), "throttle": (0.0, 1.0, 0.0, 0.0),
                        "brake": (0.0, 0.0, 1.0, 0.0), "speed": (0.0, 0.0, 0.0, 1.0)}

    @classmethod
    def _saliency_weights(cls, output):
        if isinstance(output, str):
            if output not in cls.SALIENCY_OUTPUTS:
                raise ValueError(f"saliency: unknown output {output!r} (one of "
                                 f"{sorted(cls.SALIENCY_OUTPUTS)}, or four weights)")
            return np.asarray(cls.SALIENCY_OUTPUTS[output], dtype=np.float32)
        try:
            w = np.asarray(output, dtype=np.float32)
        except (TypeError, ValueError):
            w = None
        if w is None or w.shape != (4,) or not np.isfinite(w).all():
            raise ValueError("saliency: output must be 'steer', 'throttle', 'brake', 'speed' or four "
                             "finite weights over (steer, throttle, brake, speed)")
        return w

    def _saliency_buffers(self, shape):
        """Pinned + device staging of one saliency call for frames of `shape` (cached)."""
        sal = getattr(self, "_sal", None)
        if sal is not None and sal["shape"] == shape and sal["eng"] is self.eng:
            return sal
        dev = self.eng.device
        b, h, w = self.batch, self.frames_host.size(1), self.frames_host.size(2)
        nfr = int(np.prod(shape))
        # [frames | speed | d controls | d pred_speed | command]: one H2D copy
        o_spd = (nfr + 15) // 16 * 16
        o_dc = o_spd + 4 * b
        o_ds = o_dc + 12 * b
        o_cmd = (o_ds + 4 * b + 7) // 8 * 8
        host = torch.zeros(o_cmd + 8 * b, dtype=torch.uint8).pin_memory()
        dbuf = torch.zeros_like(host, device=dev)

        def views(buf):
            return (buf[:nfr].view(shape), buf[o_spd:o_dc].view(torch.float32),
                    buf[o_dc:o_ds].view(torch.float32).view(b, 3),
                    buf[o_ds:o_ds + 4 * b].view(torch.float32),
                    buf[o_cmd:o_cmd + 8 * b].view(torch.int64))
        # [controls | pred_speed | peak | heat]: one D2H copy
        out_dev = torch.empty(b * 5 + b * h * w, dtype=torch.float32, device=dev)
        out_host = torch.zeros(b * 5 + b * h * w, dtype=torch.float32).pin_memory()
        sal = dict(shape=shape, eng=self.eng, host=host, dev=dbuf,
                   host_np=[v.numpy() for v in views(host)], dev_views=views(dbuf),
                   out_dev=out_dev, out_host=out_host, out_np=out_host.numpy(),
                   ctrl=out_dev[:3 * b].view(b, 3), spd=out_dev[3 * b:4 * b],
                   peak=out_dev[4 * b:5 * b], heat=out_dev[5 * b:].view(b, h, w),
                   dimage=torch.empty(b, 3, h, w, dtype=torch.float32, device=dev))
        self._sal = sal
        return sal

    @torch.no_grad()
    def saliency(self, frames_u8, speeds_kmh, commands, output="steer"):
        """Which pixels moved an output: (out [B,4], heat [B,H,W] float32, peak [B]).

        `out` is what predict_batch returns.  `heat` is max over the colour channels of
        |d (w . (steer, throttle, brake, pred_speed)) / d pixel| per 8-bit pixel level (the raw
        network outputs, pred_speed not yet multiplied by 90), divided by its per-frame maximum
        `peak`; `output` picks w: "steer" | "throttle" | "brake" | "speed", or four weights.
        frames: uint8 [B,88,200,3] at the network resolution, or raw camera frames [B,Hs,Ws,3|4]
        of any other size -- those are resized on the device like predict_camera does, and the
        map is over the resized frame (upscaling it for display is the caller's).  The
        eval-mode forward that keeps its graph, the data-gradient-only backward and the map
        kernel run on this predictor's stream through the per-layer plan of the same shape; the
        single-frame persistent state and later predict_batch calls are not disturbed."""
        wts = self._saliency_weights(output)                       # ValueError before any launch
        frames, speeds, cmds, camera = self._checked_frames("saliency", frames_u8, speeds_kmh,
                                                            commands)
        b, h, w = self.batch, self.frames_host.size(1), self.frames_host.size(2)

        def launch(eng, sal, pl, dc_dev, ds_dev):
            eng.run_backward(pl, dc_dev, ds_dev, data_only=True, segments=(0, 6))
            eng.run_input_grads(pl, sal["dimage"], None)
            eng.run_saliency_map(sal["dimage"], [1.0 / (255.0 * sd) for sd in IMG_STD],
                                 heat=sal["heat"], peak=sal["peak"])
        out, o, _ = self._frozen_graph_run(frames, speeds, cmds, camera, wts, launch, 5 * b + b * h * w)
        return out, o[5 * b:].reshape(b, h, w).copy(), o[4 * b:5 * b].copy()

    def _checked_frames(self, who, frames_u8, speeds_kmh, commands):
        """What `who` (saliency, gradcam) refuses of its frames, speeds and commands before
        anything is launched: returns (frames, speeds in km/h as float64, commands, whether the
        frames are camera-sized, i.e. to be resized on the device)."""
        frames = np.asarray(frames_u8)
        b = self.batch
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[0] != b or \
                frames.shape[3] not in (3, 4):
            raise RuntimeError(f"{who}: frames must be uint8 [{b},H,W,3] (camera frames: 3 or 4 "
                               "bytes per pixel)")
        camera = frames.shape[1:] != (self.frames_host.size(1), self.frames_host.size(2), 3)
        cmds = self._check_commands(commands)
        speeds = np.asarray(speeds_kmh, dtype=np.float64)
        if cmds.shape != (b,) or speeds.shape != (b,):
            raise RuntimeError(f"{who}: {b} speeds and commands expected")
        return frames, speeds, cmds, camera

    def _frozen_graph_run(self, frames, speeds, cmds, camera, wts, launch, n_out):
        """What saliency and the deeper Grad-CAM layers share: checked inputs through the pinned
        staging buffer, the eval-mode forward that keeps its graph, then launch(eng, sal, pl,
        d controls, d pred_speed) on this predictor's stream, the first n_out output floats back
        to the host, one synchronise.  Returns (out [B,4], the host outputs, launch's result)."""
        b, h, w = self.batch, self.frames_host.size(1), self.frames_host.size(2)
        if self.model.engine() is not self.eng:
            self.__init__(self.model, b, h, w, self.use_graph, self.half, self.persistent)
        if self.model.training:
            self.model.eval()
        sal = self._saliency_buffers(tuple(frames.shape))
        f_np, s_np, dc_np, ds_np, c_np = sal["host_np"]
        np.copyto(f_np, frames)
        s_np[...] = np.minimum(speeds / SPEED_NORM_FACTOR, 1.0)
        dc_np[...] = wts[:3]
        ds_np[...] = wts[3]
        c_np[...] = cmds
        f_dev, s_dev, dc_dev, ds_dev, c_dev = sal["dev_views"]
        eng = self.eng
        self._order_after_weight_updates()
        with torch.cuda.stream(self.stream):
            sal["dev"].copy_(sal["host"], non_blocking=True)
            _, _, pl = eng.run_forward_frozen_u8(f_dev, s_dev, c_dev, h if camera else None,
                                                 w if camera else None, out=(sal["ctrl"], sal["spd"]))
            res = launch(eng, sal, pl, dc_dev, ds_dev)
            sal["out_host"][:n_out].copy_(sal["out_dev"][:n_out], non_blocking=True)
            self.stream.synchronize()
        o = sal["out_np"]
        return self._result4(o[:3 * b], o[3 * b:4 * b]), o, res

    # ---- SmoothGrad / integrated gradients --------------------------------------------------------
    ATTRIBUTION_METHODS = {"smoothgrad": 0, "integrated": 1}      # CILRS_ATTR_* of the library
    # samples per pass when `chunk` is None: min(samples, this).  Measured on an MI355X, one frame,
    # 32 samples (tools/input_grad_bench.py --attribution): chunk 8 / 16 / 32
    # = 8.7 / 5.9 / 4.2 ms per SmoothGrad call
    ATTRIBUTION_CHUNK = 32

    @classmethod
    def _attribution_args(cls, method, samples, sigma, baseline, seed, chunk, frames_shape):
        """Host-side check of attribution's own arguments (ValueError before any launch):
        returns (mode, samples, sigma255, baseline uint8 array or None, seed, chunk)."""
        if not isinstance(method, str) or method not in cls.ATTRIBUTION_METHODS:
            raise ValueError(f"attribution: unknown method {method!r} (one of "
                             f"{sorted(cls.ATTRIBUTION_METHODS)})")
        mode = cls.ATTRIBUTION_METHODS[method]

        def whole(v, name, least):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < least:
                raise ValueError(f"attribution: {name} must be an integer >= {least}, got {v!r}")
            return int(v)
        samples = whole(samples, "samples", 1)
        if samples >= 1 << 24:
            raise ValueError("attribution: samples must stay below 2^24 (the midpoint rule's "
                             "(s + 0.5) / S is evaluated in float32)")
        try:
            sigma = float(sigma)
        except (TypeError, ValueError):
            sigma = float("nan")
        if not (np.isfinite(sigma) and sigma >= 0.0 and 255.0 * sigma <= 3e38):
            raise ValueError("attribution: sigma (the noise's standard deviation as a fraction of "
                             "the 8-bit range) must be finite and >= 0")
        if baseline is not None:
            if mode != cls.ATTRIBUTION_METHODS["integrated"]:
                raise ValueError("attribution: a baseline belongs to method='integrated'")
            baseline = np.asarray(baseline)
            if baseline.dtype != np.uint8 or baseline.shape != tuple(frames_shape):
                raise ValueError(f"attribution: baseline must be None (a black frame) or a uint8 "
                                 f"array of the frames' shape {tuple(frames_shape)}")
        seed = whole(seed, "seed", 0)
        if seed >= 1 << 64:
            raise ValueError("attribution: seed must fit 64 bits")
        chunk = min(samples, cls.ATTRIBUTION_CHUNK) if chunk is None else \
            min(samples, whole(chunk, "chunk", 1))
        return mode, samples, 255.0 * sigma, baseline, seed, chunk

    def _attribution_buffers(self, chunk):
        """Pinned + device staging and the device tensors of one attribution call with `chunk`
        samples per pass (cached)."""
        att = getattr(self, "_att", None)
        if att is not None and att["chunk"] == chunk and att["eng"] is self.eng:
            return att
        dev = self.eng.device
        b, h, w = self.batch, self.frames_host.size(1), self.frames_host.size(2)
        r = b * chunk
        nfr = b * h * w * 3
        # [frames | baseline | speed | d controls x r | d pred_speed x r | command]: one H2D copy
        o_base = (nfr + 15) // 16 * 16
        o_spd = o_base + o_base
        o_dc = o_spd + 4 * b
        o_ds = o_dc + 12 * r
        o_cmd = (o_ds + 4 * r + 7) // 8 * 8
        host = torch.zeros(o_cmd + 8 * b, dtype=torch.uint8).pin_memory()
        dbuf = torch.zeros_like(host, device=dev)

        def views(buf):
            return (buf[:nfr].view(b, h, w, 3), buf[o_base:o_base + nfr].view(b, h, w, 3),
                    buf[o_spd:o_dc].view(torch.float32),
                    buf[o_dc:o_ds].view(torch.float32).view(r, 3),
                    buf[o_ds:o_ds + 4 * r].view(torch.float32),
                    buf[o_cmd:o_cmd + 8 * b].view(torch.int64))
        # [controls | pred_speed | the same at the baseline | peak | total | heat | signed]: one D2H
        n_out = b * 10 + 2 * b * h * w
        out_dev = torch.empty(n_out, dtype=torch.float32, device=dev)
        out_host = torch.zeros(n_out, dtype=torch.float32).pin_memory()
        o_heat = 10 * b
        att = dict(chunk=chunk, eng=self.eng, host=host, dev=dbuf,
                   host_np=[v.numpy() for v in views(host)], dev_views=views(dbuf),
                   out_dev=out_dev, out_host=out_host, out_np=out_host.numpy(),
                   ctrl=out_dev[:3 * b].view(b, 3), spd=out_dev[3 * b:4 * b],
                   bctrl=out_dev[4 * b:7 * b].view(b, 3), bspd=out_dev[7 * b:8 * b],
                   peak=out_dev[8 * b:9 * b], total=out_dev[9 * b:10 * b],
                   heat=out_dev[o_heat:o_heat + b * h * w].view(b, h, w),
                   signed=out_dev[o_heat + b * h * w:].view(b, h, w),
                   x=torch.empty(r, 3, h, w, dtype=torch.float32, device=dev),
                   dimage=torch.empty(r, 3, h, w, dtype=torch.float32, device=dev),
                   acc=torch.empty(b, 3, h, w, dtype=torch.float32, device=dev),
                   attr=torch.empty(b, 3, h, w, dtype=torch.float32, device=dev))
        self._att = att
        return att

    @torch.no_grad()
    def attribution(self, frames_u8, speeds_kmh, commands, output="steer", method="smoothgrad",
                    samples=32, sigma=0.15, baseline=None, seed=0, chunk=None):
        """SmoothGrad or integrated gradients of one output: (out [B,4], heat [B,H,W] float32,
        peak [B], info) -- out / heat / peak shaped as `saliency` returns them.

        method="smoothgrad": the mean of saliency's gradient over `samples` noisy copies of each
        frame, Gaussian noise of standard deviation `sigma` (a fraction of the 8-bit range) added
        to the network input and drawn on the device from `seed`; heat is saliency's definition
        applied to the mean gradient, so samples=1, sigma=0 is `saliency` itself.
        method="integrated": the mean gradient over `samples` points of the straight path from
        `baseline` (None: a black frame, or uint8 frames of the same shape) to the frame, midpoint
        rule, times (frame - baseline) in the network's input units; heat = max over the colour
        channels of |attribution| / peak.  info then also holds `signed` [B,H,W] (attributions
        summed over the channels), `total` [B] (summed over the frame), `baseline_out` [B]
        (w . outputs at the baseline) and `delta` [B] = total - (w . outputs - baseline_out),
        the completeness gap (raw network outputs: pred_speed not multiplied by 90).
        frames: uint8 [B,88,200,3] at the network resolution only.  `chunk` samples per frame go
        through one forward / data-gradient pass of batch B * chunk on this predictor's stream;
        nothing per sample touches the host, and the gradient sum is the same sequential
        chain whatever `chunk` is.  The persistent single-frame state is not disturbed."""
        wts = self._saliency_weights(output)                       # ValueError before any launch
        frames = np.asarray(frames_u8)
        h, w = self.frames_host.size(1), self.frames_host.size(2)
        mode, samples, sigma255, baseline, seed, chunk = self._attribution_args(
            method, samples, sigma, baseline, seed, chunk, frames.shape)
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[0] != self.batch or \
                frames.shape[3] not in (3, 4):
            raise RuntimeError(f"attribution: frames must be uint8 [{self.batch},{h},{w},3]")
        if frames.shape[1:] != (h, w, 3):
            raise RuntimeError(f"attribution: frames must be at the network resolution "
                               f"[{self.batch},{h},{w},3]; raw camera frames are not served (there "
                               "is no stand-alone device resize to build the sample batch from) "
                               "-- resize them first, or use saliency()")
        cmds = self._check_commands(commands)
        speeds = np.minimum(np.asarray(speeds_kmh, dtype=np.float64) / SPEED_NORM_FACTOR, 1.0)
        if cmds.shape != (self.batch,) or speeds.shape != (self.batch,):
            raise RuntimeError(f"attribution: {self.batch} speeds and commands expected")
        if self.model.engine().train_precision != "fp32":
            raise RuntimeError("attribution: fp32 plans only (the model's training plan is "
                               f"{self.model.engine().train_precision}; the eval-mode graph it "
                               "differentiates needs train_precision='fp32')")
        if self.model.engine() is not self.eng:
            self.__init__(self.model, self.batch, h, w, self.use_graph, self.half, self.persistent)
        if self.model.training:
            self.model.eval()
        integrated = mode == self.ATTRIBUTION_METHODS["integrated"]
        b = self.batch
        att = self._attribution_buffers(chunk)
        f_np, b_np, s_np, dc_np, ds_np, c_np = att["host_np"]
        np.copyto(f_np, frames)
        b_np[...] = 0 if baseline is None else baseline
        s_np[...] = speeds
        dc_np[...] = wts[:3]
        ds_np[...] = wts[3]
        c_np[...] = cmds
        f_dev, b_dev, s_dev, dc_dev, ds_dev, c_dev = att["dev_views"]
        base_dev = b_dev if baseline is not None else None         # NULL: a black frame
        scale = [1.0 / (255.0 * sd) for sd in IMG_STD]
        eng = self.eng

        def per_sample(t, n):                                      # repeat_interleave, no sync
            return t.view(b, 1).expand(b, n).reshape(-1)
        self._order_after_weight_updates()
        with torch.cuda.stream(self.stream):
            att["dev"].copy_(att["host"], non_blocking=True)
            eng.run_forward_frozen_u8(f_dev, s_dev, c_dev, out=(att["ctrl"], att["spd"]))
            if integrated:
                eng.run_forward_frozen_u8(b_dev, s_dev, c_dev, out=(att["bctrl"], att["bspd"]))
            s_rep, c_rep = per_sample(s_dev, chunk), per_sample(c_dev, chunk)
            for s0 in range(0, samples, chunk):
                n = min(chunk, samples - s0)                       # a short last chunk: its own plan
                if n != chunk:
                    s_rep, c_rep = per_sample(s_dev, n), per_sample(c_dev, n)
                x, dimg = att["x"][:b * n], att["dimage"][:b * n]
                eng.run_attr_samples(f_dev, base_dev, mode, samples, s0, n, sigma255, seed, out=x)
                _, _, pl = eng.run_forward_frozen(x, s_rep, c_rep)
                eng.run_backward(pl, dc_dev[:b * n], ds_dev[:b * n], data_only=True, segments=(0, 6))
                eng.run_input_grads(pl, dimg, None)
                eng.run_attr_accumulate(dimg, att["acc"], n, first=s0 == 0)
            if integrated:
                eng.run_attr_finalize(att["acc"], f_dev, base_dev, mode, samples, scale,
                                      attr=att["attr"], signed_map=att["signed"], total=att["total"])
                eng.run_saliency_map(att["attr"], None, heat=att["heat"], peak=att["peak"])
            else:
                eng.run_attr_finalize(att["acc"], None, None, mode, samples, attr=att["attr"])
                eng.run_saliency_map(att["attr"], scale, heat=att["heat"], peak=att["peak"])
            att["out_host"].copy_(att["out_dev"], non_blocking=True)
            self.stream.synchronize()
        o = att["out_np"]
        out = self._result4(o[:3 * b], o[3 * b:4 * b])
        info = dict(method=method, samples=samples, chunk=chunk)
        hw = b * h * w
        if integrated:
            w64 = wts.astype(np.float64)
            f_x = o[:3 * b].reshape(b, 3).astype(np.float64) @ w64[:3] + o[3 * b:4 * b] * w64[3]
            f_0 = o[4 * b:7 * b].reshape(b, 3).astype(np.float64) @ w64[:3] + o[7 * b:8 * b] * w64[3]
            total = o[9 * b:10 * b].copy()
            info.update(signed=o[10 * b + hw:].reshape(b, h, w).copy(), total=total,
                        baseline_out=f_0, delta=total - (f_x - f_0))
        return out, o[10 * b:10 * b + hw].reshape(b, h, w).copy(), o[8 * b:9 * b].copy(), info

    # ---- FGSM / PGD ------------------------------------------------------------------------------
    def _adversarial_buffers(self):
        """Pinned + device staging and the attack's device tensors of one adversarial call (cached)."""
        adv = getattr(self, "_adv", None)
        if adv is not None and adv["eng"] is self.eng:
            return adv
        from .adversarial import Attack
        dev = self.eng.device
        b, h, w = self.batch, self.frames_host.size(1), self.frames_host.size(2)
        nfr = b * h * w * 3
        # [frames | speed | d controls | d pred_speed | target controls | target speed | command]
        o_spd = (nfr + 15) // 16 * 16
        o_dc = o_spd + 4 * b
        o_ds = o_dc + 12 * b
        o_tc = o_ds + 4 * b
        o_ts = o_tc + 12 * b
        o_cmd = (o_ts + 4 * b + 7) // 8 * 8
        host = torch.zeros(o_cmd + 8 * b, dtype=torch.uint8).pin_memory()
        dbuf = torch.zeros_like(host, device=dev)

        def views(buf):
            f32 = lambda a, e: buf[a:e].view(torch.float32)
            return (buf[:nfr].view(b, h, w, 3), f32(o_spd, o_dc), f32(o_dc, o_ds).view(b, 3),
                    f32(o_ds, o_tc), f32(o_tc, o_ts).view(b, 3), f32(o_ts, o_ts + 4 * b),
                    buf[o_cmd:o_cmd + 8 * b].view(torch.int64))
        adv = dict(eng=self.eng, host=host, dev=dbuf, host_np=[v.numpy() for v in views(host)],
                   dev_views=views(dbuf), attack=Attack(self.eng, b, h, w),
                   out_host=torch.zeros(11 * b, dtype=torch.float32).pin_memory(),
                   u8_host=torch.zeros(b, h, w, 3, dtype=torch.uint8).pin_memory())
        self._adv = adv
        return adv

    @torch.no_grad()
    def adversarial(self, frames_u8, speeds_kmh, commands, output="steer", eps=2.0, steps=10,
                    alpha=None, random_start=None, goal="deviate", targets=None, seed=0):
        """How far can a perturbation of at most `eps` 8-bit levels per byte move an output:
        (out_clean [B,4], out_adv [B,4], adv_frames_u8 [B,H,W,3], info) by FGSM (steps=1) or PGD.

        `output` picks w as in `saliency`.  goal="deviate" drives w . outputs away from the clean
        prediction (either side, per frame), "error" away from `targets` ([B,4] in the units of
        `out`, or [B,3] controls when w gives the speed no weight), "increase" / "decrease" push it
        one way.  alpha: the step in levels (None: eps for one step, else 2.5 * eps / steps);
        random_start: begin at a uniform point of the eps ball drawn on the device from `seed`
        (None: for "deviate" only, where the clean frame itself has no ascent direction).  For
        "deviate" and "error" the iterate with the largest |deviation| is kept, not the last one.
        out_adv is the network's output on the returned BYTES (rounded, clipped to 0..255): what a
        camera frame would give.  info: `dev` [B] = w . (outputs - reference) of the kept float
        iterate, `dev_u8` [B] the same of out_adv, `linf` [B] = max |adv - frame| in levels, and
        `steps`, `alpha`, `eps` (raw network outputs: pred_speed not multiplied by 90).
        frames: uint8 [B,88,200,3] at the network resolution only; fp32 plans only.  Everything
        runs on this predictor's stream, nothing per iteration touches the host, and the
        persistent single-frame state is not disturbed."""
        from .adversarial import attack_args
        wts = self._saliency_weights(output)                       # ValueError before any launch
        eps, steps, alpha, random_start, goal, seed = attack_args(eps, steps, alpha, random_start,
                                                                  goal, seed)
        frames = np.asarray(frames_u8)
        b, h, w = self.batch, self.frames_host.size(1), self.frames_host.size(2)
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[0] != b or \
                frames.shape[3] not in (3, 4):
            raise RuntimeError(f"adversarial: frames must be uint8 [{b},{h},{w},3]")
        if frames.shape[1:] != (h, w, 3):
            raise RuntimeError(f"adversarial: frames must be at the network resolution "
                               f"[{b},{h},{w},3]; raw camera frames are not served (the "
                               "perturbation lives in the network's input) -- resize them first")
        cmds = self._check_commands(commands)
        speeds = np.minimum(np.asarray(speeds_kmh, dtype=np.float64) / SPEED_NORM_FACTOR, 1.0)
        if cmds.shape != (b,) or speeds.shape != (b,):
            raise RuntimeError(f"adversarial: {b} speeds and commands expected")
        tgt = None
        if goal == "error":
            if targets is None:
                raise ValueError("adversarial: goal='error' needs targets")
            tgt = np.asarray(targets, dtype=np.float32)
            if tgt.shape not in ((b, 3), (b, 4)) or not np.isfinite(tgt).all():
                raise ValueError(f"adversarial: targets must be finite [{b},4] (steer, throttle, "
                                 f"brake, speed in km/h) or [{b},3]")
            if tgt.shape == (b, 3) and wts[3] != 0:
                raise ValueError("adversarial: [B,3] targets carry no speed, but `output` weighs it")
        elif targets is not None:
            raise ValueError("adversarial: targets belong to goal='error'")
        if self.model.engine().train_precision != "fp32":
            raise RuntimeError("adversarial: fp32 plans only (the model's training plan is "
                               f"{self.model.engine().train_precision}; the eval-mode graph it "
                               "differentiates needs train_precision='fp32')")
        if self.model.engine() is not self.eng:
            self.__init__(self.model, b, h, w, self.use_graph, self.half, self.persistent)
        if self.model.training:
            self.model.eval()
        adv = self._adversarial_buffers()
        f_np, s_np, dc_np, ds_np, tc_np, ts_np, c_np = adv["host_np"]
        np.copyto(f_np, frames)
        s_np[...] = speeds
        dc_np[...] = wts[:3]
        ds_np[...] = wts[3]
        tc_np[...] = 0.0 if tgt is None else tgt[:, :3]
        ts_np[...] = 0.0 if tgt is None or tgt.shape[1] == 3 else \
            tgt[:, 3] / np.float32(SPEED_NORM_FACTOR)
        c_np[...] = cmds
        f_dev, s_dev, dc_dev, ds_dev, tc_dev, ts_dev, c_dev = adv["dev_views"]
        at = adv["attack"]
        self._order_after_weight_updates()
        with torch.cuda.stream(self.stream):
            adv["dev"].copy_(adv["host"], non_blocking=True)
            at.run(f_dev, s_dev, c_dev, dc_dev, ds_dev, wts, eps, steps, alpha, random_start, goal,
                   seed, targets=(tc_dev, ts_dev) if tgt is not None else None)
            adv["out_host"].copy_(at.out, non_blocking=True)
            adv["u8_host"].copy_(at.adv_u8, non_blocking=True)
            self.stream.synchronize()
        o = adv["out_host"].numpy()
        info = dict(dev=o[8 * b:9 * b].copy(), dev_u8=o[9 * b:10 * b].copy(),
                    linf=o[10 * b:].view(np.int32).copy(), steps=steps, alpha=alpha, eps=eps)
        return (self._result4(o[:3 * b], o[3 * b:4 * b]), self._result4(o[4 * b:7 * b], o[7 * b:8 * b]),
                adv["u8_host"].numpy().copy(), info)

    def predict_controls(self, image_rgb_u8, speed_kmh, command_idx):
        """Same return tuple as the reference's predict_controls (:918-920).  Frames that are not
        already 88x200x3 go through the fused resize (predict_camera)."""
        image_rgb_u8 = np.asarray(image_rgb_u8)
        if image_rgb_u8.shape != tuple(self.frames_host.shape[1:]):
            return self.predict_camera(image_rgb_u8, speed_kmh, command_idx)
        r = self.predict_batch(image_rgb_u8[None], [speed_kmh], [command_idx])[0]
        # the reference multiplies the float32 .item() by 90.0 in Python (double)
        return (float(r[0]), float(r[1]), float(r[2]),
                float(self._spd_np[0]) * SPEED_NORM_FACTOR)

    # ---- Monte-Carlo dropout -----------------------------------------------------------------
    def _mc_args(self, samples, p, seed):
        """Validated (samples, p, seed) of the uncertainty calls; raises ValueError before any
        launch."""
        if isinstance(samples, bool) or int(samples) != samples:
            raise ValueError("samples must be an integer")
        samples = int(samples)
        if not 1 <= samples <= self.eng.MC_MAX_SAMPLES:
            raise ValueError(f"samples must be in 1..{self.eng.MC_MAX_SAMPLES}")
        if self.batch * samples > self.eng.MC_MAX_ROWS:
            raise ValueError(f"batch * samples must not exceed {self.eng.MC_MAX_ROWS}")
        if p is None:
            p = float(getattr(self.model, "dropout", 0.0))
            if p == 0.0:
                raise ValueError(
                    "the model was built with dropout=0.0 (the reference agent does so and loads a "
                    "checkpoint trained at 0.5): pass the training dropout probability as p")
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError("p must be in [0, 1)")
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must be an integer in 0..2**64-1")
        return samples, p, int(seed)

    def _tick_inputs(self, camera=False):
        """(speed, command) tensors of the tick that just ran, as its follow-ups read them.  Every
        tick stages them in pinned host memory first, and a persistent zero-copy predictor keeps
        reading them there (as its forward does, also on a degraded tick, which copies them to the
        device besides); every other predictor passes the device copies its forward read."""
        host = self.persistent and self.zero_copy
        if camera:
            cam = self._cam
            return cam[4] if host else (cam[2][2], cam[2][3])
        return (self.speed_host, self.cmd_host) if host else (self.speed_dev, self.cmd_dev)

    def _after_tick(self, launch):
        """What follows a tick: launch(eng) on this predictor's stream, on the plan the tick just
        used (the engine's last_plan from here on), into the engine's pinned buffers; one
        synchronise.  Returns what launch returned."""
        eng = self.eng
        eng.last_plan = eng.plan(self.batch, self.frames_host.size(1), self.frames_host.size(2))
        with torch.cuda.stream(self.stream):
            res = launch(eng)
            self.stream.synchronize()
        return res

    def _controls_tick(self, image_rgb_u8, speed_kmh, command_idx):
        """predict_controls (predict_camera for a frame that is not 88x200x3, else predict_batch)
        plus what its follow-ups read: (point tuple, speed, command) -- see _tick_inputs."""
        image_rgb_u8 = np.asarray(image_rgb_u8)
        camera = image_rgb_u8.shape != tuple(self.frames_host.shape[1:])
        point = self.predict_controls(image_rgb_u8, speed_kmh, command_idx)
        return (point,) + tuple(self._tick_inputs(camera))

    def _mc_run(self, speed, command, samples, p, seed, return_samples):
        """The MC launches after the tick (_after_tick).  Returns km/h-scaled copies (mean, std,
        samples)."""
        mean, std, smp = self._after_tick(lambda eng: eng.run_heads_mc(
            speed, command, samples, p, seed, return_samples, owner=self))
        scale = np.array([1.0, 1.0, 1.0, SPEED_NORM_FACTOR], dtype=np.float32)
        return (mean.numpy() * scale, std.numpy() * scale,
                smp.numpy() * scale if return_samples else None)

    @torch.no_grad()
    def predict_uncertain(self, frames_u8, speeds_kmh, commands, samples=32, p=None, seed=0,
                          return_samples=False):
        """predict_batch plus a Monte-Carlo dropout estimate of how far its outputs can be trusted:
        BatchNorm stays in eval mode, the trunk runs once, the heads run ``samples`` times under
        their training Dropout masks (include/cilrs_hip.h, cilrs_net_heads_mc).  Returns a dict of
        np.float32 arrays: "point" [B,4] (exactly predict_batch's result), "mean" and "std" [B,4]
        over the samples (std: torch's unbiased estimate), and "samples" [B,S,4] when
        return_samples is set; column 3 of each is in km/h.  ``p`` defaults to the model's dropout
        probability; a model built with dropout=0.0 must pass it.  ``seed=0`` draws the same masks
        on every tick -- a fixed ensemble without tick-to-tick flicker; vary ``seed`` for fresh
        masks.  Bad arguments raise ValueError before anything is launched."""
        samples, p, seed = self._mc_args(samples, p, seed)
        point = self.predict_batch(frames_u8, speeds_kmh, commands)
        speed, cmd = self._tick_inputs()
        mean, std, smp = self._mc_run(speed, cmd, samples, p, seed, return_samples)
        out = {"point": point, "mean": mean, "std": std}
        if return_samples:
            out["samples"] = smp
        return out

    @torch.no_grad()
    def predict_controls_uncertain(self, image_rgb_u8, speed_kmh, command_idx, samples=32, p=None,
                                   seed=0):
        """predict_controls with error bars: ((steer, throttle, brake, speed_kmh), (std_steer,
        std_throttle, std_brake, std_speed_kmh)), the first tuple being the MC-dropout mean (see
        predict_uncertain).  Frames that are not 88x200x3 go through predict_camera's path first."""
        if self.batch != 1:
            raise RuntimeError("predict_controls_uncertain is the single-frame control-loop path")
        samples, p, seed = self._mc_args(samples, p, seed)
        _point, speed, cmd = self._controls_tick(image_rgb_u8, speed_kmh, command_idx)
        mean, std, _ = self._mc_run(speed, cmd, samples, p, seed, False)
        return tuple(float(x) for x in mean[0]), tuple(float(x) for x in std[0])

    # ---- feature-space novelty --------------------------------------------------------------------
    def _novelty_check(self, density, commands, who):
        """What the novelty calls refuse before anything is launched."""
        if self.half:
            raise RuntimeError(f"{who}: fp32 predictors only (a density fitted on fp32 features does "
                               "not describe a 16-bit trunk's)")
        density.check_model(self.model, who)
        density.check_commands(self._check_commands(commands), who)

    def _novelty_run(self, command, density):
        """The score launches after the tick (_after_tick)."""
        d2 = self._after_tick(lambda eng: eng.run_novelty(command, density.mean, density.W, owner=self))
        return d2.numpy().copy()

    @torch.no_grad()
    def predict_novelty(self, frames_u8, speeds_kmh, commands, density):
        """predict_batch plus a score of how unlike the training set the frames look to the trunk:
        returns (controls [B,3], pred_speed [B] in km/h, d2 [B]), np.float32; the first two are
        exactly predict_batch's columns.  d2 is the squared Mahalanobis distance of the pooled
        features to ``density`` (a finalised cilrs_mi355.novelty.FeatureDensity; include/cilrs_hip.h,
        cilrs_net_novelty): an unchanged predict_batch -- persistent launch, degraded mode and all --
        then three small launches on this predictor's stream and one more synchronise.
        ``density.percentile(d2)`` turns it into a threshold with a meaning.  fp32 predictors only;
        a density of another feature width or command count, and a command its fit never saw,
        raise RuntimeError before anything is launched."""
        self._novelty_check(density, commands, "predict_novelty")
        out = self.predict_batch(frames_u8, speeds_kmh, commands)
        _speed, cmd = self._tick_inputs()
        d2 = self._novelty_run(cmd, density)
        return out[:, :3].copy(), out[:, 3].copy(), d2

    @torch.no_grad()
    def predict_controls_novelty(self, image_rgb_u8, speed_kmh, command_idx, density):
        """predict_controls with the novelty score: ((steer, throttle, brake, speed_kmh), d2).
        Frames that are not 88x200x3 go through predict_camera's path first."""
        if self.batch != 1:
            raise RuntimeError("predict_controls_novelty is the single-frame control-loop path")
        self._novelty_check(density, [int(command_idx)], "predict_controls_novelty")
        point, _speed, cmd = self._controls_tick(image_rgb_u8, speed_kmh, command_idx)
        return point, float(self._novelty_run(cmd, density)[0])

    # ---- nearest recorded frames --------------------------------------------------------------------
    def _neighbours_check(self, index, k, who):
        """What the neighbour calls refuse before anything is launched."""
        if self.half:
            raise RuntimeError(f"{who}: fp32 predictors only (an index of fp32 features does not "
                               "describe a 16-bit trunk's)")
        index.check_model(self.model, who)
        if index.device != self.eng.device:
            raise RuntimeError(f"{who}: the index is on {index.device}, the predictor on "
                               f"{self.eng.device}")
        return index._check_k(k)

    def _neighbours_run(self, index, k):
        """The k-NN launches after the tick (_after_tick)."""
        idx, dist = self._after_tick(
            lambda eng: eng.run_knn(index.rows, index.origin, index.W, k, owner=self))
        return idx.numpy().copy(), dist.numpy().copy()

    @torch.no_grad()
    def predict_neighbours(self, frames_u8, speeds_kmh, commands, index, k=8):
        """predict_batch plus the recorded frames the trunk finds nearest: returns (controls [B,3],
        pred_speed [B] in km/h, idx int64 [B,k], dist float32 [B,k]); the first two are exactly
        predict_batch's columns.  idx / dist are the k rows of ``index`` (a
        cilrs_mi355.neighbours.NeighbourIndex, from FramePool.index) nearest to the pooled features,
        ascending, squared distances in the index's metric (include/cilrs_hip.h, cilrs_net_knn): an
        unchanged predict_batch -- persistent launch, degraded mode and all -- then the k-NN
        launches on this predictor's stream and one more synchronise.  dist[:, -1] is the
        non-parametric novelty score; ``index.percentile`` turns it into a threshold with a meaning.
        fp32 predictors only; an index of another feature width or of a density fitted for another
        command count raises RuntimeError before anything is launched."""
        k = self._neighbours_check(index, k, "predict_neighbours")
        out = self.predict_batch(frames_u8, speeds_kmh, commands)
        idx, dist = self._neighbours_run(index, k)
        return out[:, :3].copy(), out[:, 3].copy(), idx, dist

    @torch.no_grad()
    def predict_controls_neighbours(self, image_rgb_u8, speed_kmh, command_idx, index, k=8):
        """predict_controls with the nearest recorded frames: ((steer, throttle, brake, speed_kmh),
        idx [k], dist [k]).  Frames that are not 88x200x3 go through predict_camera's path first."""
        if self.batch != 1:
            raise RuntimeError("predict_controls_neighbours is the single-frame control-loop path")
        k = self._neighbours_check(index, k, "predict_controls_neighbours")
        point, _speed, _cmd = self._controls_tick(image_rgb_u8, speed_kmh, command_idx)
        idx, dist = self._neighbours_run(index, k)
        return point, idx[0], dist[0]

    # ---- Grad-CAM --------------------------------------------------------------------------------
    GRADCAM_LAYERS ={"layer1": 1, "layer2": 2, "layer3": 3, "layer4": 4}

    @torch.no_grad()
    def gradcam(self, frames_u8, speeds_kmh, commands, output="steer", layer="layer4", want_u8=False):
        """Which region of the feature map carried an output: (out [B,4], heat [B,H,W] float32 in
        [0,1] -- or uint8 0..255 with ``want_u8`` --, cam [B,h,w] float32, peak [B]).

        Grad-CAM of trunk group ``layer`` ("layer1" .. "layer4"; 22x50, 11x25, 6x13 and 3x7 cells
        at 88x200) for y = w . (steer, throttle, brake, pred_speed), ``output`` picking w as in
        ``saliency``: cam is the signed channel-weighted sum of the group's output, peak the maximum
        of its positive part, heat that part divided by peak and interpolated bilinearly to the
        frame (include/cilrs_hip.h, cilrs_net_gradcam).  ``"layer4"`` is an unchanged predict_batch
        -- persistent launch, degraded mode and all; predict_camera for a camera-sized frame on a
        batch-1 predictor -- followed by two small launches on this predictor's stream and one more
        synchronise: cheap enough for every tick, and ``out`` is exactly predict_batch's result.
        The deeper, finer layers reuse ``saliency``'s staging: the eval-mode forward that keeps its
        graph, then the data-gradient chain down to the group's boundary only.  fp32 predictors
        only.  Bad arguments raise ValueError / RuntimeError before anything is launched."""
        wts = self._saliency_weights(output)
        if not isinstance(layer, str) or layer not in self.GRADCAM_LAYERS:
            raise ValueError(f"gradcam: unknown layer {layer!r} (one of {sorted(self.GRADCAM_LAYERS)})")
        lnum = self.GRADCAM_LAYERS[layer]
        if self.half:
            raise RuntimeError("gradcam: fp32 predictors only (a 16-bit trunk keeps 16-bit feature "
                               "maps)")
        frames, speeds, cmds, camera = self._checked_frames("gradcam", frames_u8, speeds_kmh,
                                                            commands)
        b = self.batch
        if camera and lnum == 4 and b != 1:
            raise RuntimeError("gradcam: camera-sized frames at layer4 take predict_camera's path, "
                               "which is the single-frame one")
        if lnum == 4:
            if camera:
                r = self.predict_camera(frames[0], float(speeds[0]), int(cmds[0]))
                out = np.asarray([r], dtype=np.float32)
            else:
                out = self.predict_batch(frames, speeds, cmds)
            speed, cmd = self._tick_inputs(camera)
            cam, heat, peak, u8 = self._after_tick(
                lambda eng: eng.run_gradcam(speed, cmd, wts, 4, want_u8, owner=self))
        else:
            def launch(eng, sal, pl, dc_dev, ds_dev):
                _f, s_dev, _dc, _ds, c_dev = sal["dev_views"]
                eng.run_backward(pl, dc_dev, ds_dev, data_only=True, segments=(0, 5 - lnum))
                return eng.run_gradcam(s_dev, c_dev, wts, lnum, want_u8, owner=self)
            out, _o, (cam, heat, peak, u8) = self._frozen_graph_run(frames, speeds, cmds, camera, wts,
                                                                    launch, 4 * b)
        return (out, (u8 if want_u8 else heat).numpy().copy(), cam.numpy().copy(),
                peak.numpy().copy())
