"""CPU checks of the training loop's host side (snrse/fit.py, sgmse/ema.py, sgmse/util/inference.py): the
checkpoint layout and its round trip through load_from_checkpoint, the validation-file selection, the epoch
order and accumulation schedule, and the command line.  No kernel is launched here."""
import pytest
import torch

CKPT_KEYS = {"state_dict", "hyper_parameters", "ema", "optimizer_states", "epoch", "global_step",
             "pytorch-lightning_version", "callbacks"}
EMA_KEYS = {"decay", "num_updates", "shadow_params", "collected_params"}


def _score_model():
    from sgmse.model import ScoreModel
    return ScoreModel(backbone="ncsnpp", sde="ouve", model_type="sebridge_v3", snr_conditioned="true", theta=1.5,
                      sigma_min=0.05, sigma_max=0.5, N=30, fixed_snr=0.17783, loss_type="sqrt_mse", lr=3e-4,
                      num_eval_files=7, transform_type="exponent", batch_size=2, num_frames=64)


def _snr_model():
    from sgmse.data_module import SpecsDataModule
    from sgmse.snr_estimator import SNRModel
    return SNRModel(backbone="snrnet", lr=2e-4, num_eval_files=3, data_module_cls=SpecsDataModule, base_dir="",
                    transform_type="none", batch_size=2, num_frames=64)


def _with_ema(m, num_updates=5):
    """Shadows that differ from the weights, as after a few updates."""
    m.ema.shadow_params = [p.detach() * 0.5 + 0.25 for p in m.ema._params()]
    m.ema.num_updates = num_updates
    return m


@pytest.mark.parametrize("make", [_score_model, _snr_model], ids=["ScoreModel", "SNRModel"])
def test_checkpoint_round_trip(tmp_path, make):
    """save_checkpoint -> load_from_checkpoint with the default weights_only load: state_dict bitwise, the
    hyper-parameters, the EMA decay / num_updates / shadows; the file holds exactly the Lightning keys."""
    m = _with_ema(make())
    path = str(tmp_path / "m.ckpt")
    m.save_checkpoint(path, epoch=3, global_step=17, metrics={"si_sdr": 9.25})
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert set(raw) == CKPT_KEYS
    assert set(raw["ema"]) == EMA_KEYS and raw["ema"]["collected_params"] is None
    assert raw["hyper_parameters"]["data_module_cls"] == "SpecsDataModule"
    assert raw["epoch"] == 3 and raw["global_step"] == 17 and raw["callbacks"] == {"si_sdr": 9.25}
    assert raw["optimizer_states"] == [] and isinstance(raw["pytorch-lightning_version"], str)
    m2 = type(m).load_from_checkpoint(path)
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert list(sd) == list(sd2) and len(sd) > 10
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert m2.ema.decay == m.ema.decay and m2.ema.num_updates == 5
    assert len(m2.ema.shadow_params) == len(m.ema.shadow_params)
    assert all(torch.equal(a, b) for a, b in zip(m.ema.shadow_params, m2.ema.shadow_params))
    assert m2.resume == {"epoch": 3, "global_step": 17}
    assert m2.lr == m.lr and m2.num_eval_files == m.num_eval_files and m2.loss_type == m.loss_type
    assert m2.data_module.transform_type == m.data_module.transform_type
    assert (m2.data_module.batch_size, m2.data_module.num_frames) == (2, 64)
    if make is _score_model:
        assert (m2.model_type, m2.snr_conditioned, m2.fixed_snr, m2.sigma_max) == ("sebridge_v3", "true", 0.17783, 0.5)
        assert {k: v for k, v in raw["hyper_parameters"].items() if k in m.hparams} == m.hparams


def test_checkpoint_saved_under_ema_weights_holds_the_live_weights(tmp_path):
    m = _with_ema(_snr_model())
    live = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.eval(no_ema=False)  # EMA weights swapped in
    swapped = m.state_dict()
    assert any(not torch.equal(live[k], swapped[k]) for k in live)
    path = str(tmp_path / "e.ckpt")
    m.save_checkpoint(path)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert all(torch.equal(raw["state_dict"][k], live[k]) for k in live)
    assert all(torch.equal(a, b) for a, b in zip(raw["ema"]["shadow_params"], m.ema.shadow_params))
    assert len(raw["ema"]["collected_params"]) == len(m.ema.shadow_params)  # torch_ema stores them while swapped
    m.train(True)
    assert all(torch.equal(m.state_dict()[k], live[k]) for k in live)


def test_ema_state_dict_before_the_first_update():
    """torch_ema creates the shadows as copies of the parameters: that is what an untrained model saves."""
    m = _snr_model()
    sd = m.ema.state_dict()
    assert set(sd) == EMA_KEYS and sd["num_updates"] == 0 and sd["decay"] == m.ema.decay
    assert all(torch.equal(s, p) and s.data_ptr() != p.data_ptr() for s, p in zip(sd["shadow_params"], m.ema._params()))


@pytest.mark.parametrize("total,n", [(10, 3), (7, 7), (5, -1), (1, 1)])
def test_eval_file_selection(total, n):
    from sgmse.util.inference import eval_indices
    want = torch.linspace(0, total - 1, total if n == -1 else n, dtype=torch.int).tolist()
    got = eval_indices(total, n)
    assert got == want and all(isinstance(i, int) for i in got)
    assert got[0] == 0 and got[-1] == total - 1


def test_epoch_order_and_accumulation_schedule():
    from snrse import fit
    a = fit.epoch_permutation(11, seed=3, epoch=2)
    assert sorted(a.tolist()) == list(range(11))
    import numpy as np
    np.random.seed(99)
    torch.manual_seed(99)  # global generators do not enter
    assert fit.epoch_permutation(11, seed=3, epoch=2).tolist() == a.tolist()
    assert fit.epoch_permutation(11, seed=3, epoch=3).tolist() != a.tolist()
    assert fit.epoch_permutation(11, seed=4, epoch=2).tolist() != a.tolist()
    b = fit.epoch_batches(11, 2, seed=3, epoch=2)
    assert len(b) == 5 and [i for g in b for i in g] == a.tolist()[:10]  # drop_last
    assert fit.epoch_batches(11, 2, seed=3, epoch=2, limit=3) == b[:3]
    assert fit.epoch_batches(11, 2, seed=3, epoch=2, limit=0.5) == b[:2]
    assert fit.epoch_batches(1, 2, seed=0, epoch=0) == []
    assert fit.accumulation_steps(5, 2) == [2, 4, 5]
    assert fit.accumulation_steps(4, 2) == [2, 4]
    assert fit.accumulation_steps(3, 1) == [1, 2, 3]
    assert fit.accumulation_steps(2, 8) == [2]


def test_cli_parses_train_py_flags():
    """The README command line of train.py and of train_snr_est.py."""
    from sgmse.data_module import SpecsDataModule
    from sgmse.model import ScoreModel
    from sgmse.sdes import SDERegistry
    from sgmse.snr_estimator import SNRModel
    from snrse import fit
    argv = ["--base_dir", "d/VBD", "--modeltype", "sebridge_v3", "--transform_type", "exponent", "--loss_type", "mse",
            "--gpus=1", "--sigma-max", "1.0", "--fixed_snr", "0.17783", "--snr_conditioned", "true",
            "--num_eval_files", "-1", "--max_epochs", "3", "--gradient_clip_val", "1.0",
            "--accumulate_grad_batches", "2", "--limit_train_batches", "0.25", "--limit_val_batches", "4",
            "--resume_from_checkpoint", "x.ckpt", "--ckpt_dir", "out", "--nolog"]
    parser, temp = fit.build_parser(argv)
    assert (temp.modeltype, temp.snr_conditioned, temp.sde, temp.estimator) == ("sebridge_v3", "true", "ouve", False)
    ScoreModel.add_argparse_args(parser.add_argument_group("ScoreModel"))
    SDERegistry.get_by_name(temp.sde).add_argparse_args(parser.add_argument_group("SDE"))
    SpecsDataModule.add_argparse_args(parser.add_argument_group("DataModule"))
    a = parser.parse_args(argv)
    assert (a.sigma_max, a.fixed_snr, a.num_eval_files, a.loss_type, a.base_dir) == (1.0, 0.17783, -1, "mse", "d/VBD")
    assert (a.max_epochs, a.max_steps, a.gradient_clip_val, a.accumulate_grad_batches) == (3, None, 1.0, 2)
    assert (a.limit_train_batches, a.limit_val_batches, a.check_val_every_n_epoch) == (0.25, 4, 1)
    assert (a.resume_from_checkpoint, a.ckpt_dir, a.nolog, a.gpus) == ("x.ckpt", "out", True, 1)
    assert fit._group(parser, a, "SDE")["sigma_max"] == 1.0 and "lr" in fit._group(parser, a, "ScoreModel")
    argv = ["--estimator", "--base_dir", "d/VBD", "--gpus=1", "--num_eval_files", "10", "--transform_type", "none"]
    parser, temp = fit.build_parser(argv)
    assert temp.estimator
    SNRModel.add_argparse_args(parser.add_argument_group("SNRModel"))
    SpecsDataModule.add_argparse_args(parser.add_argument_group("DataModule"))
    a = parser.parse_args(argv)
    assert (a.transform_type, a.num_eval_files, a.base_dir) == ("none", 10, "d/VBD")


@pytest.mark.parametrize("argv", [["--modeltype", "bbed"], ["--modeltype", "sebridge_v2", "--snr_conditioned", "true"],
                                  ["--modeltype", "sebridge_v3"], []])
def test_cli_refuses_unbuilt_branches_before_device_work(argv, monkeypatch):
    """The error ScoreModel._step raises, from the base arguments alone: no model is built, fit() is not reached."""
    from sgmse import model as smodel
    from snrse import fit
    m = torch.nn.Module()
    m.model_type, m.snr_conditioned = "bbed", "false"
    with pytest.raises(NotImplementedError, match="sebridge_v3"):
        fit.fit(m)
    monkeypatch.setattr(fit, "fit", lambda *a, **k: pytest.fail("fit() reached"))
    monkeypatch.setattr(smodel, "ScoreModel", lambda *a, **k: pytest.fail("a model was built"))
    with pytest.raises(NotImplementedError) as e:
        fit.main(["--base_dir", "nowhere", *argv])
    assert str(e.value) == smodel.TRAIN_UNSUPPORTED
