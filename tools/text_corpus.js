'use strict'
// Plain-text corpus for ygm_text_v1 (test tooling): what yjs 13.5.16 (the image's bundle) says a stored document says.
// For every state of four committed snapshot fixtures (tests/golden/snapshot_v135, snapshot_text_v135,
// snapshot_pending_v135, snapshot_subdoc_v135: the `u` of each row) the state is applied to a fresh Y.Doc; for every
// root name in doc.share and for one absent name the tool records
//   flat = utf8(doc.getText(name).toString())
//   deep = utf8(the walker below): yjs's own integrated document -- _start, right, deleted, countable,
//          content.constructor === Y.ContentString / Y.ContentType -- descending at a live ContentType item and
//          appending one '\n' on return unless the output is still empty or already ends in '\n'
// as hex.  The states themselves are not stored again: a set's row i belongs to row i of its input fixture, whose
// sha256 is recorded.  The edge sessions are generated here by yjs and carry their own states.
//   node tools/text_corpus.js <out.json.gz> [limit]     (limit: only the first `limit` states of each set)
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const crypto = require('crypto')
const Y = require(path.join(__dirname, 'yjs_bundle.js')).load()

const GOLDEN = path.join(__dirname, '..', 'tests', 'golden')
const SETS = ['snapshot_v135', 'snapshot_text_v135', 'snapshot_pending_v135', 'snapshot_subdoc_v135']
const ABSENT = 'no-such-root'

const { ContentString, ContentType } = (() => {   // the content constructors, from a document of the bundle's own
  const d = new Y.Doc()
  const f = d.getXmlFragment('f')
  const t = new Y.XmlText()
  f.insert(0, [t])
  t.insert(0, 'x')
  return { ContentString: t._start.content.constructor, ContentType: f._start.content.constructor }
})()

function deepText (type) {
  let out = ''
  const stack = []
  let item = type._start
  for (;;) {
    if (item === null) {
      if (!stack.length) return out
      item = stack.pop().right
      if (out.length && out[out.length - 1] !== '\n') out += '\n'
      continue
    }
    if (!item.deleted && item.countable) {
      if (item.content.constructor === ContentString) out += item.content.str
      else if (item.content.constructor === ContentType) { stack.push(item); item = item.content.type._start; continue }
    }
    item = item.right
  }
}

const hex = s => Buffer.from(s, 'utf8').toString('hex')

// [[nameHex, flatHex, deepHex], ...] for the state's roots (doc.share order) and the absent name
function rootsOf (state) {
  const doc = new Y.Doc()
  Y.applyUpdate(doc, state)
  const names = Array.from(doc.share.keys())
  names.push(ABSENT)
  return names.map(name => {
    const t = doc.getText(name)
    return [hex(name), hex(t.toString()), hex(deepText(t))]
  })
}

// ---- edge sessions: [note, state]
function edges () {
  const out = []
  const one = (note, id, f) => { const d = new Y.Doc(); d.clientID = id; f(d); out.push([note, Y.encodeStateAsUpdate(d)]) }
  const para = (frag, at, s) => { const e = new Y.XmlElement('paragraph'); frag.insert(at, [e]); if (s !== null) { const t = new Y.XmlText(); e.insert(0, [t]); t.insert(0, s) } return e }
  one('nesting 1 deep: XmlText under the fragment', 11, d => { const t = new Y.XmlText(); d.getXmlFragment('default').insert(0, [t]); t.insert(0, 'hello') })
  one('nesting 2 deep: paragraph > text, twice', 12, d => { const f = d.getXmlFragment('default'); para(f, 0, 'first'); para(f, 1, 'second') })
  one('nesting 40 deep', 13, d => {
    let p = d.getXmlFragment('default')
    for (let i = 0; i < 40; i++) { const e = new Y.XmlElement('n' + i); p.insert(0, [e]); if (i % 7 === 3) { const t = new Y.XmlText(); e.insert(0, [t]); t.insert(0, 'L' + i) } p = e }
    const t = new Y.XmlText(); p.insert(p.length, [t]); t.insert(0, 'bottom')
  })
  one('a deleted subtree between two live ones', 14, d => { const f = d.getXmlFragment('default'); para(f, 0, 'keep-a'); const e = para(f, 1, 'gone'); para(e, 1, 'gone-child'); para(f, 2, 'keep-b'); f.delete(1, 1) })
  one('an empty nested type between two full ones', 15, d => { const f = d.getXmlFragment('default'); para(f, 0, 'a'); para(f, 1, null); para(f, 2, 'b') })
  one('only empty nested types', 16, d => { const f = d.getXmlFragment('default'); para(f, 0, null); para(f, 1, null) })
  one('a string ending in \\n before a type boundary', 17, d => { const f = d.getXmlFragment('default'); para(f, 0, 'line\n'); para(f, 1, 'next'); para(f, 2, '\n'); para(f, 3, 'last') })
  {   // an emoji split by a concurrent insert between its surrogate halves
    const a = new Y.Doc(); a.clientID = 21
    const b = new Y.Doc(); b.clientID = 22
    a.getText('text').insert(0, 'a😀b')
    Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    b.getText('text').insert(2, 'X')
    a.getText('text').insert(4, 'tail')
    Y.applyUpdate(a, Y.encodeStateAsUpdate(b))
    out.push(['an emoji split by a concurrent insert', Y.encodeStateAsUpdate(a)])
  }
  one('an emoji split by a delete range', 23, d => { const t = d.getText('text'); t.insert(0, 'a😀b🎉c'); t.delete(2, 1); t.delete(4, 1) })
  one('an emoji split in a nested text', 24, d => { const f = d.getXmlFragment('default'); const e = para(f, 0, 'x😀y'); e.get(0).insert(2, 'mid'); e.get(0).delete(0, 1) })
  one('the empty root name', 25, d => { d.getText('').insert(0, 'nameless'); d.getText('other').insert(0, 'named') })
  one('a non-ASCII root name', 26, d => { d.getText('tëxt-中-😀').insert(0, 'utf8 name'); d.getText('text').insert(0, 'ascii name') })
  one('a root name of 300 bytes', 27, d => { d.getText('n'.repeat(300)).insert(0, 'long name'); d.getText('n'.repeat(299)).insert(0, 'one shorter') })
  one('a root name that is a prefix of another', 28, d => { d.getText('doc').insert(0, 'short'); d.getText('document').insert(0, 'long'); d.getText('do').insert(0, 'shorter') })
  one('a Y.Map root: values, a nested text value', 29, d => { const m = d.getMap('map'); m.set('k', 'string value'); const t = new Y.Text(); m.set('t', t); t.insert(0, 'nested under a key'); m.set('k', 'overwritten') })
  one('a Y.Array of texts, strings and numbers', 30, d => {
    const a = d.getArray('arr')
    const t1 = new Y.Text(); const t2 = new Y.Text(); const t3 = new Y.Text()
    a.insert(0, [t1, 'plain string', 7, t2, t3])
    t1.insert(0, 'one'); t3.insert(0, 'three'); a.delete(1, 1)
  })
  one('formats and embeds inside a text', 31, d => { const t = d.getText('text'); t.insert(0, 'bold', { bold: true }); t.insert(4, ' plain'); t.insertEmbed(2, { image: 'x.png' }); t.format(1, 3, { italic: true }) })
  one('a text with every character deleted', 32, d => { const t = d.getText('text'); t.insert(0, 'abcdef'); t.insert(3, 'XYZ'); t.delete(0, 9) })
  one('a string past the flat tier (70 000 bytes)', 33, d => { d.getText('text').insert(0, 'abcdefghij'.repeat(7000)) })
  {   // two peers typing into one nested text, then a lost update (pending structs)
    const a = new Y.Doc(); a.clientID = 41
    const b = new Y.Doc(); b.clientID = 42
    const log = []
    a.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    b.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    const e = para(a.getXmlFragment('default'), 0, 'shared ')
    Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    e.get(0).insert(7, 'from-a')
    b.getXmlFragment('default').get(0).get(0).insert(7, 'from-b')
    Y.applyUpdate(a, Y.encodeStateAsUpdate(b)); Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    para(a.getXmlFragment('default'), 1, 'second')
    a.getXmlFragment('default').get(1).get(0).insert(6, ' more')
    out.push(['concurrent typing in a nested text', Y.mergeUpdates(log)])
    const lost = log.slice(); lost.splice(lost.length - 2, 1)
    out.push(['the same with an update lost (pending structs)', Y.mergeUpdates(lost)])
  }
  return out
}

// --time <asks.bin>: the CPU path this replaces, on one core: per ask (tools/snapdev/textdev.cpp's input: state, root
// name, mode) a fresh Y.Doc, applyUpdate, getText(name).toString() or the walker.  One JSON line.
function timeAsks (file) {
  const b = fs.readFileSync(file)
  const n = b.readUInt32LE(0)
  const asks = []
  let p = 4
  for (let i = 0; i < n; i++) {
    const sl = b.readUInt32LE(p); const state = b.subarray(p + 4, p + 4 + sl); p += 4 + sl
    const nl = b.readUInt32LE(p); const name = b.subarray(p + 4, p + 4 + nl).toString('utf8'); p += 4 + nl
    asks.push([state, name, b.readUInt32LE(p)]); p += 4
  }
  let best = Infinity; let bytes = 0
  for (let rep = 0; rep < 3; rep++) {
    bytes = 0
    const t0 = process.hrtime.bigint()
    for (const [state, name, mode] of asks) {
      const doc = new Y.Doc()
      Y.applyUpdate(doc, state)
      const t = doc.getText(name)
      bytes += Buffer.byteLength(mode ? deepText(t) : t.toString(), 'utf8')
    }
    best = Math.min(best, Number(process.hrtime.bigint() - t0) / 1e6)
  }
  console.log(JSON.stringify({ asks: n, text_bytes: bytes, yjs_one_core_ms: Math.round(best * 100) / 100 }))
}

if (require.main === module && process.argv[2] === '--time') timeAsks(process.argv[3])
else if (require.main === module) {
  const limit = process.argv[3] ? parseInt(process.argv[3], 10) : Infinity
  const inputs = {}
  const sets = {}
  let states = 0; let roots = 0
  for (const s of SETS) {
    const raw = fs.readFileSync(path.join(GOLDEN, s + '.json.gz'))
    inputs[s + '.json.gz'] = crypto.createHash('sha256').update(raw).digest('hex')
    const rows = JSON.parse(zlib.gunzipSync(raw).toString()).rows
    sets[s] = rows.slice(0, limit).map(r => { const x = rootsOf(Buffer.from(r[0], 'hex')); states++; roots += x.length - 1; return x })
  }
  const edge = edges().map(([note, state]) => ({ note, state: Buffer.from(state).toString('hex'), roots: rootsOf(state) }))
  const doc = {
    source: 'tools/text_corpus.js (yjs 13.5.16 bundle): node tools/text_corpus.js tests/golden/text_v135.json.gz',
    absent: hex(ABSENT),
    inputs,
    sets,
    edges: edge
  }
  fs.writeFileSync(process.argv[2], zlib.gzipSync(Buffer.from(JSON.stringify(doc)), { level: 9 }))
  console.log(JSON.stringify({ states, roots, edges: edge.length }))
}

module.exports = { deepText, rootsOf }
