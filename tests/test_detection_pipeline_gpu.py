"""DetectionPipeline on the device: the batch dict of synthetic.detection_batch from decoded pixels and quads, alone, through
the Prefetcher, and into L1BalanceCELoss."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from megreader_amd._lib import call, load, ptr  # noqa: E402
from megreader_amd.data import DetectionPipeline, Prefetcher  # noqa: E402
from megreader_amd.data.device_pipeline import RGB_MEAN  # noqa: E402
from megreader_amd.decoders.seg_detector_loss import L1BalanceCELoss  # noqa: E402
from megreader_amd.synthetic import detection_batch  # noqa: E402

H, W = 64, 96
MAPS = ('gt', 'mask', 'thresh_map', 'thresh_mask')


def host_batch(seed):
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
    polygons = [np.array([[[8.5, 6.2], [60.3, 9.8], [58.1, 30.4], [6.9, 27.7]],
                          [[50.2, 35.6], [92.8, 38.1], [99.4, 58.3], [48.7, 55.9]],           # reaches over the border
                          [[10.4, 40.3], [30.6, 40.9], [30.1, 45.2], [10.8, 44.7]]]) + rng.uniform(-1, 1, (3, 4, 2)),   # too small
                np.array([[[20.7, 12.3], [80.2, 20.6], [76.5, 50.8], [16.3, 44.1]]]) + rng.uniform(-1, 1, (1, 4, 2))]
    return images, polygons, [[False, True, False], [False]]


def direct_targets(polygons, tags):
    """mr_db_targets called directly on the same quads, padded the same way."""
    dev = torch.device("cuda")
    N, G = len(polygons), max(len(p) for p in polygons)
    polys = np.zeros((N, G, 4, 2))
    flags = np.zeros((N, G), dtype=np.int32)
    for i, (p, t) in enumerate(zip(polygons, tags)):
        polys[i, :len(p)], flags[i, :len(t)] = p, t
    d_polys, d_flags = torch.from_numpy(polys).to(dev), torch.from_numpy(flags).to(dev)
    d_count = torch.tensor([len(p) for p in polygons], dtype=torch.int32, device=dev)
    records = torch.empty((N * G * load().mr_sizeof_db_record(),), dtype=torch.uint8, device=dev)
    ignore = torch.empty((N, G), dtype=torch.int32, device=dev)
    dist = torch.empty((N, G), dtype=torch.float64, device=dev)
    out = {'gt': torch.empty((N, 1, H, W), device=dev)}
    for k in MAPS[1:]:
        out[k] = torch.empty((N, H, W), device=dev)
    call("mr_db_targets", ptr(d_polys), ptr(d_count), ptr(d_flags), N, G, H, W, 8.0, 0.4, 0.3, 0.7, ptr(records), ptr(ignore),
         ptr(dist), ptr(out['gt']), ptr(out['mask']), ptr(out['thresh_map']), ptr(out['thresh_mask']))
    out['ignore_tags'] = ignore
    return out


def test_process_makes_the_detection_batch():
    images, polygons, tags = host_batch(0)
    batch = DetectionPipeline(image_size=(H, W)).process(images, polygons, tags)
    torch.cuda.synchronize()
    like = detection_batch(2, boxes=1)
    for k, v in like.items():
        assert batch[k].shape == v.shape[:-2] + (H, W) and batch[k].dtype == v.dtype and batch[k].is_cuda, k
    pixels = torch.from_numpy(np.stack(images)).double()
    expect = ((pixels - torch.tensor(RGB_MEAN, dtype=torch.float64)).float() / 255.0).permute(0, 3, 1, 2)
    assert (batch['image'].cpu() - expect).abs().max() <= 2.0 ** -24              # one float32 ulp below 0.5
    direct = direct_targets(polygons, tags)
    for k in MAPS + ('ignore_tags',):
        assert torch.equal(batch[k], direct[k]), k
    assert batch['ignore_tags'].dtype == torch.int32 and batch['ignore_tags'].cpu().tolist() == [[0, 1, 1], [0, 0, 0]]
    assert batch['gt'].sum() > 0 and batch['mask'].min() == 0 and batch['thresh_map'].max() > 0.6


def test_prefetcher_yields_the_same_batches():
    items = [host_batch(1), host_batch(2)]
    pipe = DetectionPipeline(image_size=(H, W))
    got = [{k: v.clone() for k, v in b.items()} for b in Prefetcher(items, pipe)]
    assert len(got) == 2
    for item, b in zip(items, got):
        alone = DetectionPipeline(image_size=(H, W)).process(*item)
        for k in ('image',) + MAPS + ('ignore_tags',):
            assert torch.equal(b[k], alone[k]), k


def test_loss_on_the_batch_is_finite():
    images, polygons, tags = host_batch(3)
    batch = DetectionPipeline(image_size=(H, W)).process(images, polygons, tags)
    g = torch.Generator().manual_seed(0)
    pred = {k: torch.rand((2, 1, H, W), generator=g).mul(0.98).add(0.01).cuda().requires_grad_()
            for k in ('binary', 'thresh', 'thresh_binary')}
    loss, metrics = L1BalanceCELoss()(pred, batch)
    assert torch.isfinite(loss).all() and float(loss.detach()) > 0
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in pred.values())
