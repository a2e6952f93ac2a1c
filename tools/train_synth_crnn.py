"""Train the CRNN on crops rendered by `SynthText`, then read with it: the first report that the stack learns to read.
  python tools/train_synth_crnn.py [--steps 3000] [--batch 256] [--out FILE]
Prints the loss curve (mean of every 100 steps), the greedy word accuracy on held-out rendered words (batches the training never
drew: another seed), and what `TextReader` reads on a rendered scene with the trained recogniser and a stub detector that returns
the ground-truth quads.  A report, not a test: nothing here is asserted.
  python tools/train_synth_crnn.py --augment [--steps 3000] [--batch 256] [--out FILE]
is another report in the place of that one: the A/B of the recognition augmentation (`augment_ab` below).
The word list is built into this file (no dataset, no download); the font is Pillow's built-in one."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import megreader_amd as mr  # noqa: E402
from megreader_amd.backbones import crnn_backbone  # noqa: E402
from megreader_amd.charsets import EnglishCharset  # noqa: E402
from megreader_amd.data import GlyphAtlas, SynthScenes, SynthStyle, SynthText  # noqa: E402
from megreader_amd.decoders import CRNNDecoder  # noqa: E402
from megreader_amd.ops.decode import ctc_greedy_decode  # noqa: E402
from megreader_amd.optim import FusedAdam  # noqa: E402
from megreader_amd.reader import TextReader  # noqa: E402

WORDS = """the of and to in is that for it as was with be by on not he this are or his from at which but have an had they you were
their one all we can her has there been if more when will would who so no out up into than them only its time new some could
these two may then do first any my now such like our over man me even most made after also did many before must through back
years where much your way well down should because each just those people how too little state good very make world still own
see men work long get here between both life being under never day same another know while last might us great old year off
come since against go came right used take three kernel wave lane tile cache memory matrix vector scalar thread block grid
launch stream graph queue reader writer detector decoder encoder charset lexicon beam score crop quad scene photo pixel font glyph
atlas shadow blur noise 2024 1987 42 7 100 3000 mi355x gfx950 cdna4 hbm3e rocm""".split()


class Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = crnn_backbone()
        self.decoder = CRNNDecoder(in_channels=512)

    def forward(self, x, **kw):
        return self.decoder(self.backbone(x), **kw)


class GroundTruthBoxes(object):
    """A representer that returns the quads it was given: the detector is not what this report is about."""

    def __init__(self, polygons):
        self.polygons = polygons

    def represent(self, batch, pred):
        return [p.tolist() for p in self.polygons], None


def accuracy(model, charset, gen, batches, n):
    model.eval()
    right = total = 0
    wrong = []
    with torch.no_grad():
        for _ in range(batches):
            batch = gen.batch(n)
            pred = model(batch['image'])
            ids, lengths = ctc_greedy_decode(pred[0] if isinstance(pred, (tuple, list)) else pred)
            ids, lengths = ids.cpu().numpy(), lengths.cpu().numpy()
            for k, text in enumerate(batch['text']):
                got = charset.label_to_string(ids[k, :lengths[k]])
                right += got == text.upper()
                total += 1
                if got != text.upper() and len(wrong) < 8:
                    wrong.append((text.upper(), got))
    model.train()
    return right, total, wrong


def augment_ab(args, charset, atlas, say):
    """--augment: train twice on crops rendered in a PLAIN style -- no rotation, shear, perspective, shadow, blur or noise -- once
    as rendered and once through `RecognitionAugmenter` + `augment_crops`, and read held-out crops in the default `SynthStyle`
    with both.  What the augmentation is for, on the only labelled data this repository can make: a recogniser that has seen
    upright clean words only meets slanted, blurred, noisy ones."""
    from megreader_amd.data import RecognitionAugmenter, augment_crops
    plain = SynthStyle(rotation=(0.0, 0.0), shear=(0.0, 0.0), perspective=0.0, shadow_prob=0.0, blur_sigma=(0.0, 0.0),
                       noise=(0.0, 0.0))
    size = (32, 128)
    say("%s; CRNN, bf16, FusedAdam lr %g, %d steps of %d crops at 32 x 128 rendered in a plain style, %d words; held-out crops in "
        "the default style" % (torch.cuda.get_device_name(0), args.lr, args.steps, args.batch, len(WORDS)))
    for name, aug in (("without the augmenter", None), ("with the augmenter", RecognitionAugmenter(seed=1, p=0.8))):
        torch.manual_seed(0)
        model = Model().cuda().train()
        opt = FusedAdam(model.parameters(), lr=args.lr)
        train = SynthText(charset, [atlas], WORDS, image_size=size, style=plain, seed=0)
        held_out = SynthText(charset, [atlas], WORDS, image_size=size, seed=12345)
        t0 = time.perf_counter()
        window = []
        for step in range(args.steps):
            batch = train.batch(args.batch, photos=aug is not None)
            image = batch['image']
            if aug is not None:
                table, _ = aug.sample([size] * args.batch, size, 'resize', step)
                image = augment_crops(batch['photos'], table, size, out=image)
            opt.zero_grad()
            loss, _ = model(image, targets=batch['label'], lengths=batch['length'].long(), train=True)
            loss.mean().backward()
            opt.step()
            window.append(loss.mean().detach())
            if (step + 1) % 500 == 0 or step + 1 == args.steps:
                say("  %s: steps %5d-%5d  mean loss %.4f   (%.0f s)" % (name, step + 1 - len(window), step,
                                                                       float(torch.stack(window).mean()), time.perf_counter() - t0))
                window = []
        right, total, _ = accuracy(model, charset, held_out, 8, 256)
        say("%s: greedy word accuracy on %d held-out crops in the default style: %d right = %.2f %%"
            % (name, total, right, 100.0 * right / total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--augment", action="store_true", help="the A/B report of the recognition augmentation in the place of the "
                    "default run")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_synth_crnn.py trains on the GPU; there is none")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    charset = EnglishCharset()
    atlas = GlyphAtlas.from_font(charset, size=48)
    mr.set_compute_dtype(torch.bfloat16)
    if args.augment:
        augment_ab(args, charset, atlas, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    torch.manual_seed(0)
    model = Model().cuda().train()
    opt = FusedAdam(model.parameters(), lr=args.lr)
    train = SynthText(charset, [atlas], WORDS, image_size=(32, 128), seed=0)
    held_out = SynthText(charset, [atlas], WORDS, image_size=(32, 128), seed=12345)
    say("%s; CRNN, bf16, FusedAdam lr %g, %d steps of %d rendered crops at 32 x 128, %d words, Pillow's built-in font"
        % (torch.cuda.get_device_name(0), args.lr, args.steps, args.batch, len(WORDS)))
    t0 = time.perf_counter()
    window = []
    for step in range(args.steps):
        batch = train.batch(args.batch)
        opt.zero_grad()
        loss, _ = model(batch['image'], targets=batch['label'], lengths=batch['length'].long(), train=True)
        loss.mean().backward()
        opt.step()
        window.append(loss.mean().detach())
        if (step + 1) % 100 == 0 or step + 1 == args.steps:
            say("  steps %5d-%5d  mean loss %.4f   (%.0f s)" % (step + 1 - len(window), step, float(torch.stack(window).mean()),
                                                               time.perf_counter() - t0))
            window = []
    right, total, wrong = accuracy(model, charset, held_out, 8, 256)
    say("greedy word accuracy on %d held-out rendered crops: %d right = %.2f %%" % (total, right, 100.0 * right / total))
    for want, got in wrong:
        say("  misread %r as %r" % (want, got))

    scenes = SynthScenes(charset, [atlas], WORDS, canvas=(640, 640), words_per_scene=(8, 8), seed=777,
                         style=SynthStyle(scene_height=(0.05, 0.09)))
    scene = scenes.batch(1)
    photo = scene['photos'][0].cpu().numpy()
    reader = TextReader(lambda x: torch.zeros((x.shape[0], 1) + tuple(x.shape[2:]), device=x.device), model, charset,
                        representer=GroundTruthBoxes(scene['polygons']), det_size=(640, 640), rec_size=(32, 128),
                        rectify='quad')
    found = reader.read([photo])[0]
    say("TextReader on a rendered 640 x 640 scene, ground-truth quads, the trained recogniser:")
    say("  drawn: %s" % " ".join(t.upper() for t in scene['texts'][0]))
    say("  read:  %s" % " ".join(item['text'] for item in found))
    say("  %d of %d words read right" % (sum(item['text'] == t.upper() for item, t in zip(found, scene['texts'][0])),
                                         len(scene['texts'][0])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
