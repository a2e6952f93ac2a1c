"""`SynthText` and `SynthScenes` (data/synth_text.py) on the device: the batches have the shape the recognisers are fed with and
equal the numpy restatement of the renderer bit for bit, rendered scenes go through the quad cropper and the detection pipeline
as photos do, and a CRNN trained on rendered crops of four words learns (the loss falls)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _quad_crop_ref as Q  # noqa: E402
import _synth_text_ref as R  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data import DetectionPipeline, DevicePipeline, GlyphAtlas, QuadCropper, SynthScenes, SynthStyle, SynthText  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402

CHARSET = EnglishCharset()
WORDS = ["TEXT", "MI355X", "GFX950", "READER"]


def block_atlas(seed, gh=16):
    """A legible stand-in for a font without PIL: every class is a 4 x 3 pattern of blocks drawn from its id, 10 columns wide."""
    rng = np.random.RandomState(seed)
    n = len(CHARSET)
    w = np.zeros(n, dtype=np.int32)
    w[2:] = 10
    x0 = np.concatenate([[0], np.cumsum(w)[:-1]]).astype(np.int32)
    cover = np.zeros((gh, int(w.sum())), dtype=np.uint8)
    for i in range(2, n):
        cells = rng.randint(0, 2, (4, 3)).astype(np.uint8) * 255
        cells[i % 4, i % 3] = 255
        cover[:, x0[i] + 1:x0[i] + 10] = np.kron(cells, np.ones((gh // 4, 3), dtype=np.uint8))
    return GlyphAtlas(cover, x0, w)


ATLASES = [block_atlas(1), block_atlas(2, gh=12)]


def test_synth_text_batch_has_the_pipelines_shape_and_equals_the_restatement():
    gen = SynthText(CHARSET, ATLASES, WORDS, image_size=(32, 100), seed=3)
    batch = gen.batch(8, photos=True)
    photo = np.random.RandomState(0).randint(0, 256, (20, 30, 3)).astype(np.uint8)
    like = DevicePipeline(image_size=(32, 100), charset=CHARSET).process([photo] * 8, ["AB"] * 8)
    for key in ('image', 'label', 'length'):
        assert batch[key].dtype == like[key].dtype and batch[key].shape == like[key].shape and batch[key].is_cuda, key
    assert batch['photos'].dtype == torch.uint8 and batch['photos'].shape == (8, 32, 100, 3)
    items, canvases, quads, texts = gen.plan(8, 0)
    assert batch['text'] == texts and set(texts) <= set(WORDS)
    want_u8, want_f32 = R.render(canvases, items, ATLASES, 32, 100, RGB_MEAN)
    assert np.array_equal(batch['photos'].cpu().numpy(), want_u8)
    assert np.array_equal(batch['image'].cpu().numpy().view(np.uint32), want_f32.view(np.uint32))
    label, length = batch['label'].cpu().numpy(), batch['length'].cpu().numpy()
    for k, t in enumerate(texts):
        assert np.array_equal(label[k], CHARSET.string_to_label(t, 32)) and length[k] == len(t)
        assert CHARSET.label_to_string(label[k]) == t
    again = SynthText(CHARSET, ATLASES, WORDS, image_size=(32, 100), seed=3).batch(8)
    assert torch.equal(again['image'], batch['image']) and 'photos' not in again
    assert not torch.equal(gen.batch(8)['image'], batch['image'])                   # the next batch index
    assert len(np.unique(want_u8)) > 50


def test_batches_drawn_ahead_of_the_device_keep_their_own_tables():
    """The generator runs ahead of the stream: the device is kept busy while six batches (and four scene batches) are drawn
    without a synchronisation, so every H2D copy of the staged tables is still queued when the next batches are planned.  Each
    batch must still be rendered from its own tables and carry its own labels."""
    gen = SynthText(CHARSET, ATLASES, WORDS, image_size=(32, 100), seed=11)
    scenes = SynthScenes(CHARSET, ATLASES, WORDS, canvas=(48, 96), words_per_scene=(1, 2), seed=12,
                         style=SynthStyle(scene_height=(0.25, 0.35)))
    gen.batch(4), scenes.batch(1)                           # builds the renderers; batch index 0 of each
    torch.cuda.synchronize()
    torch.cuda._sleep(400_000_000)                          # some tenths of a second of device time in front of everything below
    crops = [gen.batch(4, photos=True) for _ in range(6)]
    drawn = [scenes.batch(2) for _ in range(4)]
    torch.cuda.synchronize()
    texts = []
    for k, batch in enumerate(crops):
        items, canvases, _, want_texts = gen.plan(4, k + 1)
        want_u8, want_f32 = R.render(canvases, items, ATLASES, 32, 100, RGB_MEAN)
        assert batch['text'] == want_texts, k
        assert np.array_equal(batch['photos'].cpu().numpy(), want_u8), k
        assert np.array_equal(batch['image'].cpu().numpy().view(np.uint32), want_f32.view(np.uint32)), k
        label = batch['label'].cpu().numpy()
        assert [CHARSET.label_to_string(row) for row in label] == want_texts, k
        assert batch['length'].cpu().tolist() == [len(t) for t in want_texts], k
        texts.append(tuple(want_texts))
    assert len(set(texts)) > 1                              # the batches differ: a stale table would show
    for k, batch in enumerate(drawn):
        items, canvases, _, want_texts, _ = scenes.plan(2, k + 1)
        assert batch['texts'] == want_texts, k
        assert np.array_equal(batch['photos'].cpu().numpy(), R.render(canvases, items, ATLASES, 48, 96, RGB_MEAN)[0]), k


def test_scenes_feed_the_cropper_and_the_detection_pipeline():
    H, W = 96, 160
    style = SynthStyle(scene_height=(0.12, 0.2))
    scenes = SynthScenes(CHARSET, ATLASES, WORDS, canvas=(H, W), words_per_scene=(2, 4), seed=4, style=style)
    batch = scenes.batch(2)
    assert batch['photos'].dtype == torch.uint8 and batch['photos'].shape == (2, H, W, 3) and batch['photos'].is_cuda
    items, canvases, quads, texts, _ = scenes.plan(2, 0)
    want_u8, _ = R.render(canvases, items, ATLASES, H, W, RGB_MEAN)
    photos = batch['photos'].cpu().numpy()
    assert np.array_equal(photos, want_u8)
    assert batch['texts'] == texts and [len(p) for p in batch['polygons']] == [len(t) for t in texts]
    assert sum(len(t) for t in texts) >= 4
    for p, tags in zip(batch['polygons'], batch['ignore_tags']):
        assert p.dtype == np.float64 and p.shape[1:] == (4, 2) and tags.dtype == bool and not tags.any()
    # the ground-truth quads through the cropper, from the resident photos and from their host copies: the restatement's crops
    cropper = QuadCropper(image_size=(32, 128), rectify='quad')
    for source in ([batch['photos'][k] for k in range(2)], [photos[k] for k in range(2)]):
        crops = cropper.crop(source, batch['polygons'])
        assert crops['image'].shape == (sum(len(t) for t in texts), 3, 32, 128) and not crops['dropped']
        index = crops['index'].cpu().numpy()
        staged, layout = cropper.pack(source, batch['polygons'])
        for m, plan in enumerate(layout.plans):
            want = Q.quad_crop_ref(photos[index[m]], plan)
            assert np.array_equal(crops['image'][m].cpu().numpy().view(np.uint32), want.view(np.uint32)), m
    # the crops hold text, not a flat ground
    assert float(crops['image'].std()) > 0.01
    pipe = DetectionPipeline(image_size=(H, W))
    out = pipe.process([photos[k] for k in range(2)], batch['polygons'], batch['ignore_tags'])
    assert out['image'].shape == (2, 3, H, W)
    want = (photos.astype(np.float64) - np.array(RGB_MEAN)).astype(np.float32) / np.float32(255)
    assert np.array_equal(out['image'].cpu().numpy(), want.transpose(0, 3, 1, 2))
    assert float(out['gt'].sum()) > 0                                               # the shrunk text regions are not empty


def test_scenes_on_resident_background_photos():
    H, W = 64, 96
    rng = np.random.RandomState(8)
    grounds = [torch.from_numpy(rng.randint(0, 256, (H + 5, W + 7, 3)).astype(np.uint8)).cuda() for _ in range(2)]
    scenes = SynthScenes(CHARSET, ATLASES, WORDS, canvas=(H, W), words_per_scene=(1, 2), seed=6, backgrounds=grounds,
                         style=SynthStyle(scene_height=(0.2, 0.3)))
    batch = scenes.batch(3)
    items, canvases, quads, texts, back = scenes.plan(3, 0)
    canvases["photo"] = 1
    want_u8, _ = R.render(canvases, items, ATLASES, H, W, RGB_MEAN, {s: grounds[int(back[s])].cpu().numpy() for s in range(3)})
    assert np.array_equal(batch['photos'].cpu().numpy(), want_u8)


def test_a_crnn_learns_to_read_four_rendered_words():
    """60 eager steps at N = 32 on crops of four words: the mean loss of the last ten steps is below the mean of the first ten.
    Any working training path meets this by a wide margin; a failure is a finding about the generator or the step."""
    from megreader_amd.backbones import crnn_backbone
    from megreader_amd.decoders import CRNNDecoder
    from megreader_amd.optim import FusedAdam

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = crnn_backbone()
            self.decoder = CRNNDecoder(in_channels=512)

        def forward(self, x, **kw):
            return self.decoder(self.backbone(x), **kw)

    torch.manual_seed(0)
    model = Model().cuda().train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    gen = SynthText(CHARSET, ATLASES, WORDS, image_size=(32, 128), seed=9)
    losses = []
    for step in range(60):
        batch = gen.batch(32)
        opt.zero_grad()
        loss, _ = model(batch['image'], targets=batch['label'], lengths=batch['length'].long(), train=True)
        loss.mean().backward()
        opt.step()
        losses.append(float(loss.mean().detach()))
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print("CRNN on rendered crops: mean loss of steps 0-9 %.4f, of steps 50-59 %.4f" % (first, last))
    assert np.isfinite(losses).all() and last < first
