"""The recognition augmentation through its front ends -- DevicePipeline, EncodedDevicePipeline, QuadCropper, Prefetcher and the
direct call `augment_crops` -- against the numpy restatement (tests/_rec_augment_ref.py), bit for bit: the augmented rows are what
the restatement gives for the descriptors the planner draws at that batch index, every other row is what the same front end
writes without an augmenter."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _rec_augment_ref as R  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data import (DevicePipeline, EncodedDevicePipeline, Prefetcher, QuadCropper, RecognitionAugmenter,  # noqa: E402
                                augment_crops)

SIZE = (32, 128)
CS = EnglishCharset()
SHAPES = [(40, 150), (23, 61), (32, 128), (64, 40), (31, 200), (48, 97), (20, 333), (36, 90)]
WORDS = ["hello", "World", "a1b2", "", "megreader", "x", "ROCm", "text"]


def augmenter(**kw):
    return RecognitionAugmenter(**dict(dict(seed=7, p=0.6, motion_prob=0.5, erase_prob=0.5, pixelate_prob=0.3), **kw))


def samples(seed, n):
    rng = np.random.RandomState(seed)
    return ([rng.randint(0, 256, SHAPES[(seed + k) % len(SHAPES)] + (3,)).astype(np.uint8) for k in range(n)],
            [WORDS[(seed + 3 * k) % len(WORDS)] for k in range(n)])


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def expected(images, plain, index, mode='resize', **kw):
    """(bits [n, 3, H, W], rows): `plain` with the rows the planner augments at `index` replaced by the restatement."""
    table, rows = augmenter(**kw).sample([im.shape for im in images], SIZE, mode, index)
    return R.batch_ref(table, images, len(images), *SIZE, before=bits(plain)), rows


@pytest.mark.parametrize("mode", ["resize", "pad"])
def test_device_pipeline(mode):
    images, texts = samples(1, 8)
    plain = DevicePipeline(SIZE, mode, CS).process(images, texts)
    pipe = DevicePipeline(SIZE, mode, CS, augmenter=augmenter())
    first, second = pipe.process(images, texts), pipe.process(images, texts)          # batch indices 0 and 1
    assert pipe.index == 2
    for index, got in ((0, first), (1, second)):
        want, rows = expected(images, plain['image'], index, mode)
        assert 0 < len(rows) < 8
        assert np.array_equal(bits(got['image']), want)
        assert not np.array_equal(bits(got['image'])[rows], bits(plain['image'])[rows])
        assert torch.equal(got['label'], plain['label']) and torch.equal(got['length'], plain['length'])
    assert not np.array_equal(bits(first['image']), bits(second['image']))
    again = pipe.upload(*pipe.pack(images, texts, index=0))                              # index= overrides the counter
    assert pipe.index == 2 and np.array_equal(bits(again['image']), bits(first['image']))
    nothing = DevicePipeline(SIZE, mode, CS, augmenter=augmenter(p=0.0)).process(images, texts)
    assert np.array_equal(bits(nothing['image']), bits(plain['image']))


def test_encoded_pipeline_equals_the_pipeline_on_its_decoded_pixels():
    from PIL import Image
    rng = np.random.RandomState(5)
    blobs = []
    for k, (h, w) in enumerate(SHAPES[:6]):
        yy, xx = np.mgrid[0:h, 0:w]
        im = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) * 3 % 256)], axis=-1) + rng.randint(-20, 20, (h, w, 3))
        buf = io.BytesIO()
        Image.fromarray(np.clip(im, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=90)
        blobs.append(buf.getvalue())
    texts = WORDS[:6]
    enc = EncodedDevicePipeline(SIZE, 'resize', CS, augmenter=augmenter())
    staged, layout = enc.pack(blobs, texts, index=3)
    got = enc.upload(staged, layout)
    pixels = [p.cpu().numpy() for p in enc.photos(got, layout)]
    assert [p.shape[:2] for p in pixels] == SHAPES[:6]
    ref = DevicePipeline(SIZE, 'resize', CS, augmenter=augmenter())
    want = ref.upload(*ref.pack(pixels, texts, index=3))
    assert np.array_equal(bits(got['image']), bits(want['image']))
    assert torch.equal(got['label'], want['label']) and torch.equal(got['length'], want['length'])
    plain = EncodedDevicePipeline(SIZE, 'resize', CS).process(blobs, texts)
    restated, rows = expected(pixels, plain['image'], 3)
    assert 0 < len(rows) < 6 and np.array_equal(bits(got['image']), restated)


def test_quad_cropper_augments_word_crops_from_a_scene():
    photo = np.random.RandomState(9).randint(0, 256, (120, 200, 3)).astype(np.uint8)
    quads = [[[10, 12], [90, 20], [88, 48], [8, 40]], [[110, 60], [190, 52], [193, 85], [113, 93]],
             [[20, 70], [45, 70], [45, 115], [20, 115]]]                    # the last one is tall: its frame is rotated
    plain_cropper = QuadCropper(SIZE)
    plain = plain_cropper.crop([photo], [quads])
    plans = plain_cropper.pack([photo], [quads])[1].plans
    assert len(plans) == 3 and plans[2].rotated
    aug = augmenter(seed=3)
    for source in (photo, torch.from_numpy(photo).cuda()):                  # staged, and resident in its own allocation
        cropper = QuadCropper(SIZE, augmenter=aug)
        for index in (0, 1):
            got = cropper.crop([source], [quads])
            table, rows = aug.sample(plans, SIZE, 'resize', index, images=[0, 0, 0])
            assert (table["cu0"] < 0).all()                                  # context around the word
            want = R.batch_ref(table, [photo], 3, *SIZE, before=bits(plain['image']))
            assert np.array_equal(bits(got['image']), want)
            assert torch.equal(got['index'], plain['index']) and torch.equal(got['quad'], plain['quad'])
        assert cropper.index == 2
    counts = [len(aug.sample(plans, SIZE, 'resize', index, images=[0, 0, 0])[1]) for index in (0, 1)]
    assert 0 < sum(counts) < 6                                               # some rows augmented, some left as QuadCropper() writes them


def test_prefetcher_draws_ahead_of_a_busy_device():
    """Six batches are packed while the prefetch stream is still busy with what was queued before them, so every copy of a
    staged table is still to run when the next tables are drawn: each batch must come out of its own tables."""
    batches = [samples(20 + k, 6) for k in range(6)]
    plain_pipe = DevicePipeline(SIZE, 'resize', CS)
    plain = [plain_pipe.process(*b)['image'] for b in batches]
    pipe = DevicePipeline(SIZE, 'resize', CS, augmenter=augmenter())
    pipe.process(*batches[0])                                                # warm: the buffers and the kernels exist
    pipe.index = 0
    torch.cuda.synchronize()
    fetch = Prefetcher(batches, pipe)
    with torch.cuda.stream(fetch.stream):
        torch.cuda._sleep(200_000_000)                                       # device time in front of everything below
    got = [(b['image'], b['label']) for b in fetch]                          # no synchronisation, no clone
    torch.cuda.synchronize()
    assert len(got) == 6 and pipe.index == 6
    for k, (images, texts) in enumerate(batches):
        want, rows = expected(images, plain[k], k)
        assert np.array_equal(bits(got[k][0]), want), "batch %d" % k
        assert torch.equal(got[k][1], plain_pipe.process(images, texts)['label'])


def test_augment_crops_on_device_resident_crops():
    images, _ = samples(4, 5)
    device = [torch.from_numpy(im).cuda() for im in images]
    device[2] = torch.from_numpy(np.pad(images[2], ((0, 0), (0, 5), (0, 0)))).cuda()[:, :images[2].shape[1]]    # a padded pitch
    plain = DevicePipeline(SIZE, 'resize', CS).process(images, [""] * 5)['image']
    table, rows = augmenter(p=0.5, seed=2).sample([im.shape for im in images], SIZE, 'resize', 0)
    assert 0 < len(rows) < 5
    got = augment_crops(device, table, SIZE)
    assert np.array_equal(bits(got), R.batch_ref(table, images, 5, *SIZE, before=bits(plain)))
    out = torch.full((7, 3) + SIZE, float('nan'), device="cuda")
    moved = table.copy()
    moved["row"] += 2
    assert augment_crops(device, moved, SIZE, out=out) is out
    want = R.batch_ref(moved, images, 7, *SIZE, before=bits(out.clone().fill_(float('nan'))))
    assert np.array_equal(bits(out), want) and torch.isnan(out[0]).all()
    for bad in (dict(row=7), dict(image=5)):
        broken = moved.copy()
        broken[list(bad)[0]][0] = list(bad.values())[0]
        with pytest.raises(ValueError):
            augment_crops(device, broken, SIZE, out=out)
    with pytest.raises(TypeError):
        augment_crops([torch.from_numpy(images[0])], table[:0], SIZE)
