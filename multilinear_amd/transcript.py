"""Transcript (src/transcript.rs) over the C ABI (host SHA-256 in libmlhip)."""
import ctypes

from .device import check, context, fe_from_bytes, lib, ptr


class Transcript:
    """transcript.rs:5-38: running SHA-256; random() finalizes a clone;
    next_challenge() = F::from(u128_le(random()[..16])) without absorbing."""

    def __init__(self, _handle=None):
        if _handle is None:
            h = ctypes.c_void_p()
            check(lib().mlh_transcript_create(ctypes.byref(h)))
            _handle = h.value
        self.h = _handle

    def __del__(self):
        try:
            lib().mlh_transcript_destroy(self.h)
        except Exception:
            pass

    def clone(self):
        h = ctypes.c_void_p()
        check(lib().mlh_transcript_clone(self.h, ctypes.byref(h)))
        return Transcript(h.value)

    def absorb(self, data: bytes):
        buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data) if data else None
        check(lib().mlh_transcript_absorb(self.h, buf, len(data)))

    def random(self) -> bytes:
        out = (ctypes.c_uint8 * 32)()
        check(lib().mlh_transcript_random(self.h, out))
        return bytes(out)

    def next_challenge(self) -> int:
        out = (ctypes.c_uint8 * 16)()
        check(lib().mlh_transcript_next_challenge(self.h, out))
        return fe_from_bytes(out)


class DeviceTranscript:
    """The transcript state in HBM (mlh_transcript_to_device): device kernels
    absorb device bytes and write next_challenge() to device memory, with no
    host round trip.  A copy of a host Transcript (a fresh one by default);
    to_host() copies the state back.  Tensor arguments live on `device`."""

    def __init__(self, transcript=None, device=0):
        import torch

        self.device = device
        self.state = torch.empty(int(lib().mlh_device_transcript_bytes()), dtype=torch.uint8,
                                 device="cuda:%d" % device)
        self.load(transcript if transcript is not None else Transcript())

    def load(self, transcript: Transcript):
        ctx = context(self.device)
        check(lib().mlh_transcript_to_device(ctx, transcript.h, ptr(self.state)), ctx)

    def to_host(self, transcript=None) -> Transcript:
        """The state as a host Transcript (`transcript` is overwritten, or a new one made)."""
        tr = transcript if transcript is not None else Transcript()
        ctx = context(self.device)
        check(lib().mlh_transcript_from_device(ctx, ptr(self.state), tr.h), ctx)
        return tr

    def absorb(self, src, challenge_out=None, nbytes=None):
        """absorb the bytes of device tensor `src` (its first `nbytes`; src may
        be None for 0 bytes); next_challenge() -> challenge_out (a (1, 4) int32
        element) unless None."""
        n = src.numel() * src.element_size() if nbytes is None else nbytes
        ctx = context(self.device)
        check(lib().mlh_device_transcript_absorb(
            ctx, ptr(self.state), ptr(src) if src is not None else None, n,
            ptr(challenge_out) if challenge_out is not None else None), ctx)

    def fri_last(self, vals2, flag_out, last_out):
        """The final FRI layer vals2 (2 elements): flag_out (one uint32) =
        (vals2[0] != vals2[1]), last_out = vals2[0], absorb LE16(vals2[0])."""
        ctx = context(self.device)
        check(lib().mlh_device_fri_last(ctx, ptr(vals2), ptr(self.state), ptr(flag_out),
                                        ptr(last_out)), ctx)

    def sumcheck_round(self, sum_pairs, npairs, prev, poly_out, r_out):
        """One sumcheck round from `npairs` partial (p(1), p(2)) pairs and the
        claim `prev`: poly_out = (c1, c2), absorbed; r_out = next_challenge();
        prev = p(r_out)."""
        ctx = context(self.device)
        check(lib().mlh_device_sumcheck_round(ctx, ptr(sum_pairs), npairs, ptr(prev),
                                              ptr(self.state), ptr(poly_out), ptr(r_out)), ctx)
