"""TEST INFRASTRUCTURE — the row-by-row loop of src/extract_playlist.py:4-28 over four parallel lists, with the one
change n2v_hip/playlist.py documents: the reference reads row idx+1 on the last row of the file (an IndexError); here
the last row has no successor and ends its session.  The product never imports this file."""


def extract_playlist(uid, timestamp, playtime, tid):
    n = len(uid)

    def continues(idx):                    # row idx+1 belongs to the session of row idx
        return (idx + 1 < n and uid[idx + 1] == uid[idx]
                and int(timestamp[idx + 1]) < int(timestamp[idx]) + int(playtime[idx]) + 300)

    sentence_list, temp_sentence, idx = [], [], 0
    while idx < n:
        while continues(idx):
            if int(playtime[idx]) > 9:
                temp_sentence.append(tid[idx])
            idx = idx + 1
        temp_sentence.append(tid[idx])
        idx = idx + 1
        sentence_list.append(temp_sentence)
        temp_sentence = []
    return [x for x in sentence_list if len(x) > 1]
