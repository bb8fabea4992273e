"""YUV4MPEG2 (.y4m) streams: the container raw YUV frames travel in through a pipe (`ffmpeg -f yuv4mpegpipe`, mpv, x264).

    YUV4MPEG2 W832 H480 F16:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\\n
    FRAME\\n <one frame's planes> FRAME\\n ...

The header and every FRAME line are ASCII, space-separated tags ended by a newline; a frame is Y, U, V planes as
`yuv_reference` lays out i420 / i422 / i444 / gray.  The tag spellings here (C420jpeg / C420mpeg2 / C420paldv / C420, C422,
C444, Cmono, the deeper C420p10 ..., C444alpha, the interlace letters and ffmpeg's XCOLORRANGE extension) are quoted from
memory of the format's description and of ffmpeg's muxer; they are not checked against an ffmpeg checkout, which the build
machine does not have.  The three 4:2:0 tags differ in where chroma is sited; this project's filters treat all of them as
centre-sited."""
from __future__ import annotations

import os
from fractions import Fraction
from typing import BinaryIO, Iterable, Iterator, Optional, Union

from . import yuv_reference as yr

MAGIC = b"YUV4MPEG2"
COLOUR_TAGS = {"420jpeg": "i420", "420mpeg2": "i420", "420paldv": "i420", "420": "i420", "422": "i422", "444": "i444", "mono": "gray"}
_WRITE_TAGS = {"i420": "420jpeg", "i422": "422", "i444": "444", "gray": "mono"}
_MAX_LINE = 4096


def _open(path_or_file, mode: str):
    """(file object, whether this module opened it)."""
    if isinstance(path_or_file, (str, bytes, os.PathLike)):
        return open(path_or_file, mode, buffering=0 if "r" in mode else -1), True
    return path_or_file, False


class Y4mReader:
    """Iterates over the frames (`bytes`, `yuv_reference.frame_bytes(fmt, height, width)` each) of a YUV4MPEG2 file, pipe or
    file object.  It reads exactly what it is asked for -- the header when it is made, one FRAME line and one frame per
    `next` -- so a FIFO or /dev/stdin is a live source.  `width`, `height`, `fps` (a Fraction), `fmt`, `range`
    ("limited" unless the header says XCOLORRANGE=FULL) and `header` (the raw tags) describe the stream."""

    def __init__(self, path_or_file: Union[str, os.PathLike, BinaryIO]):
        self._f, self._own = _open(path_or_file, "rb")
        try:
            self._parse_header(self._line("the stream header"))
        except Exception:
            self.close()
            raise

    # ------------------------------------------------------------------------------------------
    def _read(self, n: int) -> bytes:
        """Up to n bytes, short only at the end of the stream (a pipe or raw file returns what it has)."""
        parts, got = [], 0
        while got < n:
            b = self._f.read(n - got)
            if not b:
                break
            parts.append(b)
            got += len(b)
        return b"".join(parts)

    def _line(self, what: str) -> Optional[bytes]:
        """One line without its newline, byte by byte (nothing beyond it is consumed); None at a clean end of stream."""
        out = bytearray()
        while True:
            c = self._f.read(1)
            if not c:
                if out:
                    raise ValueError(f"y4m: the stream ends inside {what}: {bytes(out)!r}")
                return None
            if c == b"\n":
                return bytes(out)
            out += c
            if len(out) > _MAX_LINE:
                raise ValueError(f"y4m: {what} is longer than {_MAX_LINE} bytes; not a YUV4MPEG2 stream")

    def _parse_header(self, line: Optional[bytes]) -> None:
        if line is None or not line.startswith(MAGIC):
            raise ValueError(f"y4m: not a YUV4MPEG2 stream (it starts with {(line or b'')[:16]!r})")
        self.header = line[len(MAGIC):].decode("ascii", "replace").split()
        self.width = self.height = None
        self.fps, self.fmt, self.range = Fraction(0), "i420", "limited"
        for tag in self.header:
            key, val = tag[0], tag[1:]
            if key in "WH":
                if not val.isdigit() or int(val) < 1:
                    raise ValueError(f"y4m: bad size tag {tag!r}")
                setattr(self, "width" if key == "W" else "height", int(val))
            elif key == "F":
                num, _, den = val.partition(":")
                if not (num.isdigit() and den.isdigit()):
                    raise ValueError(f"y4m: bad frame rate tag {tag!r}")
                self.fps = Fraction(int(num), int(den)) if int(den) else Fraction(0)
            elif key == "I":
                if val not in ("p", "?"):
                    raise ValueError(f"y4m: interlaced streams are not taken (tag {tag!r}; only Ip and I? are)")
            elif key == "C":
                if val not in COLOUR_TAGS:
                    raise ValueError(f"y4m: colour space tag {tag!r} is not taken (8-bit {', '.join('C' + t for t in COLOUR_TAGS)} are)")
                self.fmt = COLOUR_TAGS[val]
            elif key == "X" and val.startswith("COLORRANGE="):
                r = val.partition("=")[2]
                if r not in ("FULL", "LIMITED"):
                    raise ValueError(f"y4m: bad colour range tag {tag!r}")
                self.range = r.lower()
        if self.width is None or self.height is None:
            raise ValueError(f"y4m: the header has no W or no H tag: {self.header}")
        self.frame_bytes = yr.frame_bytes(self.fmt, self.height, self.width)
        self.frames_read = 0

    # ------------------------------------------------------------------------------------------
    def __iter__(self) -> Iterator[bytes]:
        return self

    def __next__(self) -> bytes:
        if self._f is None:
            raise StopIteration
        line = self._line(f"the FRAME line of frame {self.frames_read}")
        if line is None:
            self.close()
            raise StopIteration
        if line != b"FRAME" and not line.startswith(b"FRAME "):                 # "FRAME Ixxx ...": parameters are allowed and ignored
            raise ValueError(f"y4m: expected a FRAME line for frame {self.frames_read}, got {line[:32]!r}")
        data = self._read(self.frame_bytes)
        if len(data) != self.frame_bytes:
            raise ValueError(f"y4m: frame {self.frames_read} is truncated: {len(data)} of {self.frame_bytes} bytes")
        self.frames_read += 1
        return data

    def close(self) -> None:
        if self._f is not None and self._own:
            self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4mWriter:
    """`write(frames)` appends raw frames (`bytes`) to a YUV4MPEG2 file, pipe or file object; the header goes out with the
    first write, and every call flushes, so a reader on the other end of a pipe sees the frames as they are written."""

    def __init__(self, path_or_file: Union[str, os.PathLike, BinaryIO], width: int, height: int, fps, fmt: str = "i420", range: str = "limited"):
        if fmt not in _WRITE_TAGS:
            raise ValueError(f"y4m has no tag for {fmt!r} (it carries {', '.join(_WRITE_TAGS)}); nv12 and the packed formats are not y4m formats")
        if range not in yr.RANGES:
            raise ValueError(f"range must be 'full' or 'limited', got {range!r}")
        self.frame_bytes = yr.frame_bytes(fmt, height, width)       # ValueError for a bad size
        fps = Fraction(fps)
        if fps <= 0:
            raise ValueError(f"fps must be positive, got {fps}")
        self.width, self.height, self.fps, self.fmt, self.range = int(width), int(height), fps, fmt, range
        self._f, self._own = _open(path_or_file, "wb")
        self._header_written = False
        self.frames_written = 0

    def header(self) -> bytes:
        return (f"YUV4MPEG2 W{self.width} H{self.height} F{self.fps.numerator}:{self.fps.denominator} Ip A1:1 C{_WRITE_TAGS[self.fmt]} "
                f"XCOLORRANGE={self.range.upper()}\n").encode("ascii")

    def write(self, frames: Iterable[bytes]) -> int:
        """Frames written by this call."""
        if isinstance(frames, (bytes, bytearray, memoryview)):
            frames = [frames]
        if not self._header_written:
            self._f.write(self.header())
            self._header_written = True
        count = 0
        for f in frames:
            if len(f) != self.frame_bytes:
                raise ValueError(f"y4m: frame {self.frames_written} has {len(f)} bytes, a {self.height}x{self.width} {self.fmt} frame {self.frame_bytes}")
            self._f.write(b"FRAME\n")
            self._f.write(f)
            self.frames_written += 1
            count += 1
        self._f.flush()
        return count

    def close(self) -> None:
        if self._f is not None:
            if not self._header_written:                            # an empty stream is still a stream
                self._f.write(self.header())
                self._header_written = True
            self._f.flush()
            if self._own:
                self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
