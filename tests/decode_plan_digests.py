"""SHA-256 of the descriptor blocks the two planners write (jpeg.DecodePlan, png.DecodePlan) for the small fixtures: what
tests/golden/decode_plan_digests.json records (tools/make_decode_plan_digests.py) and tests/test_decoder_frontend_cpu.py compares.  Uses the public
names only, so that it runs unchanged on any commit that has both decoders.  Host only.

Per fixture (one file per plan) the block is planned without outputs and with one made-up, non-null output in each form that fits the file; the
planner stores those pointers and never follows them.  jpeg_dec is planned serially and with ``parallel=True``, jpeg_prog with ``progressive=True``.
Per set, the whole set is also planned as one batch, without outputs and with planar outputs."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLDEN, "decode_plan_digests.json")
OUT, TABLE = 0x7f0000100000, 0x7f0000200000                     # made up: 16-byte aligned, never dereferenced


def _files(stem, suffix):
    with open(os.path.join(GOLDEN, stem + ".json")) as f:
        names = [c["name"] for c in json.load(f)["cases"]]
    z = np.load(os.path.join(GOLDEN, stem + ".npz"))
    return [(n, z[n + suffix].tobytes()) for n in names]


def _sets():
    from livespeechportraits_amd import jpeg as J
    from livespeechportraits_amd import png as P
    return (("jpeg_dec", J, _files("jpeg_dec", ".jpg"), {}), ("jpeg_dec_parallel", J, _files("jpeg_dec", ".jpg"), {"parallel": True}),
            ("jpeg_prog", J, _files("jpeg_prog", ".jpg"), {"progressive": True}), ("png_dec", P, _files("png_dec", ".png"), {}))


def _sha(plan):
    return hashlib.sha256(plan.blob[:int(plan.bytes)].tobytes()).hexdigest()


def _spec(info, form, k=0):
    """(ptr, table, plane_stride, form) for file k of a batch"""
    planar = form == 2
    return (OUT + 0x1000000 * k, TABLE if planar else 0, info.width * info.height if planar else 0, form)


def digests():
    """{"<set>/<fixture>/<none | rgb8 | gray8 | planar>": sha256, "<set>/batch/<none | planar>": sha256}"""
    out = {}
    for name, mod, files, kw in _sets():
        infos = []
        for fixture, data in files:
            plan = mod.DecodePlan([data], **kw)
            info = plan.file(0)
            assert info.status == 0, (name, fixture)
            infos.append(info)
            out["%s/%s/none" % (name, fixture)] = _sha(plan)
            first = ("rgb8", mod.FORM_RGB8) if info.components == 3 else ("gray8", mod.FORM_GRAY8)
            for label, form in (first, ("planar", mod.FORM_PLANAR_F32)):
                out["%s/%s/%s" % (name, fixture, label)] = _sha(mod.DecodePlan([data], outputs=[_spec(info, form)], **kw))
        batch = [data for _, data in files]
        out["%s/batch/none" % name] = _sha(mod.DecodePlan(batch, **kw))
        out["%s/batch/planar" % name] = _sha(mod.DecodePlan(batch, outputs=[_spec(i, mod.FORM_PLANAR_F32, k) for k, i in enumerate(infos)], **kw))
    return out
