"""``det`` CLI verbs that the reference's command tree has and no other test covers: ``auth`` and
``oauth`` against an in-process master."""

import pytest


def test_auth_and_oauth_verbs(capsys):
    from determined_amd.cli import main
    from determined_amd.master import start_master

    srv = start_master()
    try:
        url = f"http://127.0.0.1:{srv.port}"
        main(["-m", url, "auth", "list-providers"])
        assert "No SSO providers found." in capsys.readouterr().out
        main(["-m", url, "auth", "login"])
        assert "No SSO providers found." in capsys.readouterr().out
        with pytest.raises(SystemExit):
            main(["-m", url, "oauth", "client", "list"])
    finally:
        srv.stop()
        srv.master.close()
