"""CPU-only checks of the soft Dice loss's surface: host-side argument validation of the C entries (nothing
is launched), the no-CPU-fallback rule, and the opt-in wiring (train.py --loss, the trainers' loss=)."""
import os

import pytest
import torch


def test_softdice_entries_reject_bad_arguments_without_gpu():
    """Null pointers, K = 9 and a bad flag return PMU_ERR_ARG before any launch; the workspace query is a
    host function: 0 for a shape the kernels refuse, and it grows with the per-image block count."""
    from pmu_hip._lib import LIB_PATH, PMU_ERR_ARG, load_library
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    cdll = load_library()
    p = 4096   # a non-null address: never dereferenced, the argument checks return first
    assert cdll.pmu_softdice_fwd(None, None, 2, 3, 64, 0, 0, 0, -100, None, None, None) == PMU_ERR_ARG
    assert cdll.pmu_softdice_bwd(None, None, 2, 3, 64, 0, 0, -100, None, None, None, None) == PMU_ERR_ARG
    assert cdll.pmu_softdice_fwd(p, p, 2, 9, 64, 0, 0, 0, -100, p, p, None) == PMU_ERR_ARG
    assert cdll.pmu_softdice_bwd(p, p, 2, 9, 64, 0, 0, -100, p, p, p, None) == PMU_ERR_ARG
    assert cdll.pmu_softdice_fwd(p, p, 2, 3, 64, 2, 0, 0, -100, p, p, None) == PMU_ERR_ARG    # act
    assert cdll.pmu_softdice_fwd(p, p, 2, 3, 64, 0, 0, 2, -100, p, p, None) == PMU_ERR_ARG    # first_class
    assert cdll.pmu_softdice_fwd(p, p, 0, 3, 64, 0, 0, 0, -100, p, p, None) == PMU_ERR_ARG    # N
    assert cdll.pmu_softdice_fwd(p, p, 2, 3, 64, 0, 0, 0, -100, p, p + 4, None) == PMU_ERR_ARG  # ws alignment
    assert cdll.pmu_softdice_ws(2, 9, 64) == 0 and cdll.pmu_softdice_ws(0, 3, 64) == 0
    # coefficients (float N K 2) + sums (double N (3K + 1)) + one partial row per block
    assert cdll.pmu_softdice_ws(2, 3, 64) == 2 * 3 * 2 * 4 + 2 * 10 * 8 + 2 * 1 * 10 * 8
    assert cdll.pmu_softdice_ws(2, 3, 3 * 2048) == 2 * 3 * 2 * 4 + 2 * 10 * 8 + 2 * 3 * 10 * 8
    assert cdll.pmu_softdice_ws(4, 2, 1 << 30) == 4 * 2 * 2 * 4 + 4 * 7 * 8 + 4 * 256 * 7 * 8   # 1024 blocks at most


def test_soft_dice_loss_refuses_cpu_tensors():
    from pmu_hip.loss import SoftDiceLoss
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SoftDiceLoss()(torch.rand(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        from dice_loss import dice_loss
        dice_loss(torch.rand(2, 1, 4, 4), torch.rand(2, 1, 4, 4))


def test_soft_dice_loss_constructor_defaults():
    from pmu_hip.loss import SoftDiceLoss
    m = SoftDiceLoss()
    assert (m.include_background, m.per_image, m.ignore_index, m.from_logits) == (True, False, -100, None)
    m = SoftDiceLoss(False, True, 255, True)
    assert (m.include_background, m.per_image, m.ignore_index, m.from_logits) == (False, True, 255, True)


def test_train_parser_loss_flag():
    import train as T
    assert T.get_args([]).loss == "default"
    assert T.get_args(["--loss", "dice"]).loss == "dice"
    assert T.get_args(["--loss", "ce+dice", "-m", "probunet"]).loss == "ce+dice"
    with pytest.raises(SystemExit):
        T.get_args(["--loss", "foo"])


def test_trainers_reject_unknown_loss():
    """A bad loss= raises before the network is built, so this needs no GPU."""
    from pmu_hip.loss import BCELoss, CEPlusDiceLoss, CrossEntropyLoss, SoftDiceLoss, make_criterion
    from trainer import ProbUNetTrainer, UNetTrainer
    with pytest.raises(ValueError):
        UNetTrainer(torch.device("cpu"), n_classes=3, num_filters=[4, 8], loss="foo")
    with pytest.raises(ValueError):
        ProbUNetTrainer(torch.device("cpu"), n_classes=3, num_filters=[4, 8], loss="foo")
    assert type(make_criterion(1)) is BCELoss and type(make_criterion(3)) is CrossEntropyLoss
    assert type(make_criterion(3, "dice")) is SoftDiceLoss
    both = make_criterion(1, "ce+dice")
    assert type(both) is CEPlusDiceLoss and type(both.criterion) is BCELoss and type(both.dice) is SoftDiceLoss


def test_probabilistic_unet_recon_loss_defaults():
    """The constructor's positional surface is unchanged; recon_loss / dice_weight trail it."""
    import inspect
    from model import ProbabilisticUnet
    names = list(inspect.signature(ProbabilisticUnet.__init__).parameters)
    assert names == ["self", "input_channels", "num_classes", "num_filters", "latent_dim", "no_convs_fcomb", "beta",
                     "recon_loss", "dice_weight"]
    d = inspect.signature(ProbabilisticUnet.__init__).parameters
    assert d["recon_loss"].default == "ce" and d["dice_weight"].default == 1.0
