"""The front end the JPEG and the PNG decoder share (livespeechportraits_amd/imagedec.py), without a device: which decoder load_candidates hands
which files in which calls, that the two decoders and plans are subclasses that redefine none of the shared methods, the error text, and that the
descriptor blocks of both planners are byte for byte those of the commit before the front end was shared (tests/golden/decode_plan_digests.json)."""
import json
import sys

import pytest
import torch

import decode_plan_digests as G
import jpeg_decode_cases as JK
import png_decode_cases as PK

SIZE = 64


class _Decoder:
    """stands in for a decoder: records (kind.method, file indices, channel0) and hands `decode`'s callers one tagged tensor per file"""

    def __init__(self, kind, files, log):
        self.kind, self.files, self.log = kind, files, log

    def decode_into(self, files, out, channel0, table):
        assert tuple(out.shape) == (12, SIZE, SIZE) and tuple(table.shape) == (256,)
        self.log.append((self.kind + ".decode_into", tuple(self.files.index(f) for f in files), channel0))

    def decode(self, files):
        idx = tuple(self.files.index(f) for f in files)
        self.log.append((self.kind + ".decode", idx, None))
        return [torch.full((1,), j) for j in idx]


class _Resizer:
    def __init__(self, log):
        self.log = log

    def resize_planes(self, pixels, size, table, out, filt):
        assert size == SIZE and tuple(out.shape) == (3, SIZE, SIZE) and filt == "bicubic"
        self.log.append(("resize", (int(pixels[0]), ), out.storage_offset() // (SIZE * SIZE)))


@pytest.fixture(scope="module")
def sources():
    """four different files of each kind: J / P are 64 x 64 RGB, j / p are RGB of another size"""
    jpegs, pngs = JK.fixtures()[1], PK.fixtures()[1]
    text = lambda data, j: PK._insert(data, b"IEND", b"tEXt", b"n\0%d" % j)            # an ancillary chunk: the same image, other bytes
    return {"J": [jpegs["candidate_%d_64x64_q95" % j] for j in range(4)], "j": [jpegs[JK.find(n)] for n in ("smooth_420_47x33", "extremes_444_47x33", "primaries_422_47x33", "sparse_opt_47x33")],
            "P": [text(pngs["rgb_64x64"], j) for j in range(4)], "p": [text(pngs["rgb_65x65"], j) for j in range(4)]}


def _into(kind, idx):
    return (kind + ".decode_into", tuple(idx), 3 * idx[0])


def _resampled(kind, j):
    return [(kind + ".decode", (j, ), None), ("resize", (j, ), 3 * j)]


J, P = "jpeg", "png"
# pattern (J, P: a 64 x 64 file of that kind; j, p: one of another size), png=, resize=, the calls in order
ROUTES = [
    ("PPPP", True, None, [_into(P, (0, 1, 2, 3))]),
    ("JJJJ", True, None, [_into(J, (0, 1, 2, 3))]),
    ("JJPP", True, None, [_into(J, (0, 1)), _into(P, (2, 3))]),
    ("PJPJ", True, None, [_into(P, (0, )), _into(J, (1, )), _into(P, (2, )), _into(J, (3, ))]),
    ("PPPP", True, "bicubic", [_into(P, (0, 1, 2, 3))]),
    ("PJPJ", True, "bicubic", [_into(P, (0, )), _into(J, (1, )), _into(P, (2, )), _into(J, (3, ))]),
    ("jJJJ", True, "bicubic", [_into(J, (1, 2, 3))] + _resampled(J, 0)),
    ("JjJJ", True, "bicubic", [_into(J, (0, )), _into(J, (2, 3))] + _resampled(J, 1)),
    ("JJjJ", True, "bicubic", [_into(J, (0, 1)), _into(J, (3, ))] + _resampled(J, 2)),
    ("JJJj", True, "bicubic", [_into(J, (0, 1, 2))] + _resampled(J, 3)),
    ("pPPP", True, "bicubic", [_into(P, (1, 2, 3))] + _resampled(P, 0)),
    ("PPpP", True, "bicubic", [_into(P, (0, 1)), _into(P, (3, ))] + _resampled(P, 2)),
    ("PpJJ", True, "bicubic", [_into(P, (0, )), _into(J, (2, 3))] + _resampled(P, 1)),
    ("JPPp", True, "bicubic", [_into(J, (0, )), _into(P, (1, 2))] + _resampled(P, 3)),
    ("pJjP", True, "bicubic", [_into(J, (1, )), _into(P, (3, ))] + _resampled(P, 0) + _resampled(J, 2)),
    ("jjjj", True, "bicubic", [(J + ".decode", (0, 1, 2, 3), None)] + [("resize", (j, ), 3 * j) for j in range(4)]),
    # png=False: every file is the JPEG decoder's, a PNG among them (it refuses it)
    ("JJJJ", False, None, [_into(J, (0, 1, 2, 3))]),
    ("PJPJ", False, None, [_into(J, (0, 1, 2, 3))]),
    ("PPPP", False, None, [_into(J, (0, 1, 2, 3))]),
    ("JJJJ", False, "bicubic", [_into(J, (0, 1, 2, 3))]),
    ("jjjj", False, "bicubic", [(J + ".decode", (0, 1, 2, 3), None)] + [("resize", (j, ), 3 * j) for j in range(4)]),
    # png=False with files to resample: neighbouring files that need none go in one call, as with png=True (before, one call per file)
    ("jJJJ", False, "bicubic", [_into(J, (1, 2, 3))] + _resampled(J, 0)),
    ("JjJJ", False, "bicubic", [_into(J, (0, )), _into(J, (2, 3))] + _resampled(J, 1)),
    ("JJjJ", False, "bicubic", [_into(J, (0, 1)), _into(J, (3, ))] + _resampled(J, 2)),
    ("JJJj", False, "bicubic", [_into(J, (0, 1, 2))] + _resampled(J, 3)),
    ("PjPJ", False, "bicubic", [_into(J, (0, )), _into(J, (2, 3))] + _resampled(J, 1)),
]
GROUPED = [r for r in ROUTES if not r[1] and r[2] and any(c in "jp" for c in r[0]) and any(c in "JP" for c in r[0])]


@pytest.mark.parametrize("pattern,png,resize,calls", ROUTES, ids=["%s-png%d-%s" % (r[0], r[1], r[2]) for r in ROUTES])
def test_load_candidates_routes_each_file_to_its_decoder(sources, pattern, png, resize, calls, monkeypatch):
    """The table above was written first and run against the commit before load_candidates had one body: every row agrees with it except the five
    of GROUPED (png=False, resize=, some files to resample and some not), where that commit made one decode_into call per file and this one groups
    neighbours as png=True always did.  With png=False the png module is not needed: the import is made to fail here."""
    from livespeechportraits_amd.candidates import load_candidates
    assert len(GROUPED) == 5
    files = [sources[c][k] for k, c in enumerate(pattern)]
    assert len(set(files)) == 4
    log = []
    if not png:
        import livespeechportraits_amd
        monkeypatch.delattr(livespeechportraits_amd, "png", raising=False)
        monkeypatch.setitem(sys.modules, "livespeechportraits_amd.png", None)
    got = load_candidates(files, device="cpu", size=SIZE, decoder=_Decoder(J, files, log), png_decoder=_Decoder(P, files, log), resizer=_Resizer(log),
                          resize=resize, png=png)
    assert tuple(got.shape) == (1, 12, SIZE, SIZE) and got.dtype == torch.float32
    assert log == calls


# ---- the shape of the front end ----------------------------------------------------------------------------------------------------------------
SHARED = ("_buffer", "_run", "_infos", "decode", "decode_into")


def test_both_decoders_are_subclasses_that_redefine_nothing_shared():
    from livespeechportraits_amd import imagedec, jpeg, png
    for mod, dec in ((jpeg, jpeg.JpegDecoder), (png, png.PngDecoder)):
        assert issubclass(dec, imagedec.Decoder) and issubclass(mod.DecodePlan, imagedec.DecodePlan)
        assert not [name for name in SHARED if name in dec.__dict__]
        assert not [name for name in ("file", "statuses") if name in mod.DecodePlan.__dict__]
        assert (mod.FORM_RGB8, mod.FORM_GRAY8, mod.FORM_PLANAR_F32) == (0, 1, 2) and mod._aligned is imagedec._aligned
    assert issubclass(jpeg.JpegError, imagedec.DecodeError) and issubclass(png.PngError, imagedec.DecodeError) and issubclass(imagedec.DecodeError, ValueError)
    for name in ("qtable", "segment", "parallel_segment", "parallel_stats", "scans", "host_coefficients"):
        assert name in jpeg.DecodePlan.__dict__
    assert "host_scanlines" in png.DecodePlan.__dict__ and "host_pixels" in png.DecodePlan.__dict__
    from livespeechportraits_amd import candidates
    assert not hasattr(candidates, "_load_candidates_mixed")


def test_the_errors_keep_their_text():
    from livespeechportraits_amd import jpeg, png
    e = jpeg.JpegError([0, 2, 1])
    assert str(e) == "JPEG file 1 of the batch is CORRUPT (refused files: 1: CORRUPT, 2: UNSUPPORTED)"
    assert isinstance(e, ValueError) and (e.statuses, e.index, e.code) == ([0, 2, 1], 1, 2)
    assert str(jpeg.JpegError([3, 0, 7])) == "JPEG file 0 of the batch is RANGE (refused files: 0: RANGE, 2: 7)"
    e = png.PngError([0, 2, 1])
    assert str(e) == "PNG file 1 of the batch is CORRUPT (refused files: 1: CORRUPT, 2: UNSUPPORTED)"
    assert isinstance(e, ValueError) and (e.statuses, e.index, e.code) == ([0, 2, 1], 1, 2)
    assert str(png.PngError([3])) == "PNG file 0 of the batch is 3 (refused files: 0: 3)"
    for mod, dec, kind in ((jpeg, jpeg.JpegDecoder, "JPEG"), (png, png.PngDecoder, "PNG")):
        with pytest.raises(RuntimeError) as r:
            dec("cpu")
        assert str(r.value) == "the %s decoder runs on the MI355X only (no CPU path); the reference's host path is cv2.imread / Pillow" % kind


# ---- the descriptor blocks ------------------------------------------------------------------------------------------------------------------
def test_descriptor_blocks_are_byte_for_byte_the_recorded_ones():
    """every small fixture of jpeg_dec (serial and parallel=True), jpeg_prog (progressive=True) and png_dec, one file per plan, without outputs and
    with a made-up output in each form that fits, and each set as one batch: the SHA-256 of blob[:bytes] is the one recorded from the commit before
    this front end (tools/make_decode_plan_digests.py; two runs there gave equal digests, so no byte of a block is left unset)"""
    with open(G.PATH) as f:
        want = json.load(f)
    got = G.digests()
    assert len(want) > 1000 and sorted(got) == sorted(want)
    assert not sorted(k for k in want if got[k] != want[k])
